// pekf_magcal_resume.hip -- phase 1 fed in chunks (pekf_magcal_resume_dev, pekf_magcal_state_bytes): k_magcal
// (pekf_magcal.hip) on the next rows of the same phones' phase-1 plane, in a file of its own so that
// pekf_magcal.hip's object holds the kernels it held.
//
// What carries over is what the reference's Magnetometer_Calibration object holds between two messages
// (KFS/Magnetometer_Calibration.cpp:7-36): x[100] y[100] z[100], the running bias sum, num_rows and isCalibrated.
// The sums alone do not do, as they do for chunked phase 2: the fit needs the n_cal samples a second time,
// centred on a bias that is known only at message n_cal + 1 (setUncalibratedValues, :65-80), so the samples are
// kept on the device.  When a phone's message n_cal + 1 arrives its lane fits from the store -- pass 2's body
// and the solve are pekf_magcal.hpp's, k_magcal's own -- and writes its outputs once.  The store's layout is
// MagcalState (pekf_magcal.hpp).
#include "pekf_magcal.hpp"

namespace pekf {

constexpr int kMcFitRing = 8;  // stored samples in flight per firing lane (pass 2)

// k_magcal's pass 1, statement for statement, on rows that continue a phone's stream, and for the lanes whose
// count passes n_cal in this launch k_magcal's pass 2 (over the stored samples, in slot order = arrival order)
// and its solve.  resume == 0: the sums and counts start at zero and every phone's outputs are first written as
// not calibrated; resume != 0: from `state`.  The null events that pad a chunk's last block, time events and FP64
// no-message events are not messages and move nothing.
template <bool EV64>
__global__ __launch_bounds__(kMcBlock) void k_magcal_resume(int64_t batch, int64_t n_events,
                                                            const std::conditional_t<EV64, double4, float4> *__restrict__ ev,
                                                            int n_cal, double *cal, double *fit, int32_t *status,
                                                            void *state, int32_t resume) {
    using EvT = std::conditional_t<EV64, double4, float4>;
    const int64_t b = (int64_t)blockIdx.x * kMcBlock + threadIdx.x;
    if (b >= batch) return;
    const uint32_t lane = (uint32_t)b;
    const int32_t n_ev = (int32_t)n_events;  // < 2^30, checked on the host: the uniform tests stay scalar
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int cnt = 0;
    if (resume) {
        const double2 h0 = *state_plane(state, batch, b, 0), h1 = *state_plane(state, batch, b, 1);
        sx = h0.x; sy = h0.y; sz = h1.x;
        cnt = __double2loint(h1.y);
        if (__all(cnt > n_cal)) return;  // every phone of the wave fired in an earlier launch: nothing is read
    } else {
        const double w[3][3] = {}, xs[6] = {};
        magcal_store(b, 1, 0.0, 0.0, 0.0, w, xs, cal, fit, status);  // not calibrated: bias 0, W = I, fit NaN
    }
    const bool fired_before = cnt > n_cal;
    // pass 1 (setValues, :13-43): the sum of the first n_cal samples, each kept in its slot; the lane counts its
    // messages up to n_cal + 1, the one that fires the fit
    for (int32_t e0 = 0; e0 < n_ev; e0 += kMcRing) {
        if (__all(cnt > n_cal)) break;
        EvT r[kMcRing];
        load_event_block<kMcRing, kMcNtl>(ev, batch, lane, e0, n_ev, r);  // padded with null events: no messages
#pragma unroll
        for (int k = 0; k < kMcRing; ++k) {
#pragma clang fp contract(off)
            const EvT v4 = r[k];
            if (!is_message(v4)) continue;
            if (cnt < n_cal) {
                sx += (double)v4.x;
                sy += (double)v4.y;
                sz += (double)v4.z;
                *MagcalState::sample(state, batch, b, cnt, 0) = (double)v4.x;
                *MagcalState::sample(state, batch, b, cnt, 1) = (double)v4.y;
                *MagcalState::sample(state, batch, b, cnt, 2) = (double)v4.z;
            }
            if (cnt <= n_cal) ++cnt;
        }
    }
    *state_plane(state, batch, b, 0) = make_double2(sx, sy);
    *state_plane(state, batch, b, 1) = make_double2(sz, __hiloint2double(0, cnt));
    if (fired_before || cnt <= n_cal) return;  // written once, in the launch that holds message n_cal + 1

    const double bx = sx / (double)n_cal, by = sy / (double)n_cal, bz = sz / (double)n_cal;  // :20-22
    // pass 2: the normal equations of the n_cal stored samples, centred (setUncalibratedValues, :65-80)
    double ata[21] = {}, atb[6] = {};
    for (int k0 = 0; k0 < n_cal; k0 += kMcFitRing) {
        double s[kMcFitRing][3];
#pragma unroll
        for (int k = 0; k < kMcFitRing; ++k) {  // slots past the last: the last again (read only)
            const int slot = k0 + k < n_cal ? k0 + k : n_cal - 1;
#pragma unroll
            for (int c = 0; c < 3; ++c) s[k][c] = *MagcalState::sample(state, batch, b, slot, c);
        }
#pragma unroll
        for (int k = 0; k < kMcFitRing; ++k) {
            if (k0 + k >= n_cal) break;  // uniform
            magcal_add_row(s[k][0], s[k][1], s[k][2], bx, by, bz, ata, atb);
        }
    }
    magcal_solve_store(b, true, bx, by, bz, ata, atb, cal, fit, status);
}

}  // namespace pekf

using namespace pekf;

static bool magcal_flags_ok(uint32_t flags) { return (flags & ~(PEKF_EV_TIME_EVENTS | PEKF_EV_F64_EVENTS)) == 0; }

static_assert(sizeof(long long) == sizeof(int64_t), "pekf_magcal_state_bytes returns 64 bits");
extern "C" long long int pekf_magcal_state_bytes(int64_t batch, int n_cal, uint32_t flags) {
    if (batch < 0 || n_cal < 6 || n_cal >= (1 << 30) || !magcal_flags_ok(flags)) return -1;
    return batch * (long long)MagcalState::bytes_per_phone(n_cal);
}

extern "C" int pekf_magcal_resume_dev(int64_t batch, int64_t n_events, const void *ev_planes, int n_cal, double *cal,
                                      double *fit, int32_t *status, uint32_t flags, void *state, int resume,
                                      void *stream) {
    PEKF_CHECK_ARG(batch >= 0 && n_events >= 0, "negative size");
    PEKF_CHECK_ARG(n_cal >= 6 && n_cal < (1 << 30), "n_cal must be >= 6 (the fit has 6 unknowns) and < 2^30");
    PEKF_CHECK_ARG(n_events < ((int64_t)1 << 30), "n_events must be < 2^30 per launch");
    PEKF_CHECK_ARG(magcal_flags_ok(flags), "unknown flags");
    PEKF_CHECK_ARG(state && (uintptr_t)state % 16 == 0, "state must be a 16-byte aligned pointer");
    if (batch == 0) return PEKF_OK;
    PEKF_CHECK_ARG(batch < ((int64_t)1 << 28), "batch must be < 2^28 phones per launch");
    PEKF_CHECK_ARG((ev_planes || n_events == 0) && cal && status, "null pointer");
    PEKF_CHECK_ARG((uintptr_t)ev_planes % 16 == 0, "misaligned event planes");
    const dim3 grid(grid_for(batch, kMcBlock)), block(kMcBlock);
    dispatch_bools(
        [&](auto ev64) {  // time events are always honoured, as in phase 2
            using Ev = std::conditional_t<ev64.value, double4, float4>;
            hipLaunchKernelGGL(k_magcal_resume<ev64.value>, grid, block, 0, as_stream(stream), batch, n_events,
                               static_cast<const Ev *>(ev_planes), n_cal, cal, fit, status, state,
                               (int32_t)(resume != 0));
        },
        (flags & PEKF_EV_F64_EVENTS) != 0);
    return launched("k_magcal_resume");
}
