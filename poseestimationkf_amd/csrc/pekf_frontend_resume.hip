// pekf_frontend_resume.hip -- phase 2 fed in chunks (pekf_frontend_init_resume_dev,
// pekf_frontend_init_state_bytes): k_frontend_init's first pass (pekf_frontend.hip; pekf_phase2.hpp) on the next
// rows of the same phones' phase-2 plane, its per-phone running state (InitState, pekf_phase2.hpp) kept in a device
// buffer between launches, in a file of its own so that pekf_frontend.hip's object and listing hold the kernels
// they held.  The means alone: the reference's variance is a second pass over the first n_avg samples once the
// mean is known, and a chunked feed no longer has them.
#include "pekf_phase2.hpp"

namespace pekf {

// k_frontend_init's first pass, statement for statement (pekf_phase2.hpp says why it is not one function), on
// rows that continue a phone's stream: resume == 0 starts from t_start as the one launch does, resume != 0 from
// `state`.  The null events that pad a chunk's last block of rows fall mid-stream here and move nothing: an FP64
// no-message event is skipped, the f32 one is a time event of step 0.  The outputs are the one launch's on the
// rows fed so far.
template <bool EV64>
__global__ __launch_bounds__(kInitBlock) void k_frontend_init_resume(
    int64_t batch, int64_t n_events, const std::conditional_t<EV64, double4, float4> *__restrict__ ev,
    const int64_t *__restrict__ t_start, int n_avg, double *__restrict__ init, int64_t *__restrict__ t_init,
    int32_t *__restrict__ ready, void *__restrict__ state, int32_t resume) {
    using EvT = std::conditional_t<EV64, double4, float4>;
    const int64_t b = (int64_t)blockIdx.x * kInitBlock + threadIdx.x;
    if (b >= batch) return;
    const uint32_t lane = (uint32_t)b;
    double sum[3][3] = {};  // [type][xyz]
    int cnt[3] = {0, 0, 0};
    bool done[3] = {false, false, false};  // Acc_ / Gyr_ / Mag_initialized
    bool kalman = false;                   // the KalmanFilter is built
    int64_t t, t_last;
    // (the counts pass through copies: handed to load / store itself, the array indexed by the event's type
    // was placed in LDS, 12 B per lane, where k_frontend_init keeps it in registers)
    if (resume) {
        int c[3];
        InitState::load(state, batch, b, sum, c, done, kalman, t, t_last);
        cnt[0] = c[0]; cnt[1] = c[1]; cnt[2] = c[2];
    } else {
        t = t_last = t_start[b];
    }
    const int32_t n_ev = (int32_t)n_events;
    for (int32_t e0 = 0; e0 < n_ev; e0 += kInitRing) {
        EvT r[kInitRing];
        load_event_block<kInitRing, PEKF_INIT_NTL>(ev, batch, lane, e0, n_ev, r);
#pragma unroll
        for (int k = 0; k < kInitRing; ++k) {
            const EvT v4 = r[k];
            const int ty = (int)event_type(v4);
            if constexpr (EV64) {
                if (!is_message(v4)) continue;
                t = (int64_t)ev64_time(v4);
            } else {
                if (!is_message(v4)) {  // a time event: the clock moves, nothing else happens
                    t += (int64_t)time_step(v4);
                    continue;
                }
                t += (int64_t)(__float_as_uint(v4.w) >> 2);
            }
            if (!(done[0] && done[1] && done[2])) {
                if (ty <= 2) {
                    if (cnt[ty] < n_avg) {
                        sum[ty][0] += (double)v4.x;
                        sum[ty][1] += (double)v4.y;
                        sum[ty][2] += (double)v4.z;
                        ++cnt[ty];
                    } else {
                        done[ty] = true;
                    }
                }
            } else {
                kalman = true;  // the KalmanFilter is built at the first such event, later ones move its time
                t_last = t;
            }
        }
    }
    const int cs[3] = {cnt[0], cnt[1], cnt[2]};
    InitState::store(state, batch, b, sum, cs, done, kalman, t, t_last);
    const double nan = __builtin_nan("");
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        init[6 * b + j] = kalman ? sum[kEvAcc][j] / (double)n_avg : nan;
        init[6 * b + 3 + j] = kalman ? sum[kEvMag][j] / (double)n_avg : nan;
    }
    t_init[b] = t_last;
    ready[b] = kalman ? 1 : 0;
}

}  // namespace pekf

using namespace pekf;

static_assert(sizeof(long long) == sizeof(int64_t), "pekf_frontend_init_state_bytes returns 64 bits");
extern "C" long long int pekf_frontend_init_state_bytes(int64_t batch, uint32_t flags) {
    if (batch < 0 || !init_flags_ok(flags)) return -1;
    return batch * (long long)InitState::kBytes;
}

extern "C" int pekf_frontend_init_resume_dev(int64_t batch, int64_t n_events, const void *ev_planes,
                                             const int64_t *t_start, int n_avg, double *init, int64_t *t_init,
                                             int32_t *ready, uint32_t flags, void *state, int resume, void *stream) {
    if (int st = check_init_args(batch, n_events, n_avg, flags, ev_planes, init, t_init, ready)) return st;
    PEKF_CHECK_ARG(state && (uintptr_t)state % 16 == 0, "state must be a 16-byte aligned pointer");
    if (batch == 0) return PEKF_OK;
    PEKF_CHECK_ARG(batch < ((int64_t)1 << 28), "batch must be < 2^28 phones per launch");
    PEKF_CHECK_ARG(resume || t_start, "null pointer");  // read when a session starts
    const dim3 grid(grid_for(batch, kInitBlock)), block(kInitBlock);
    dispatch_bools(
        [&](auto ev64) {  // phase 2 always honours time events
            using Ev = std::conditional_t<ev64.value, double4, float4>;
            hipLaunchKernelGGL(k_frontend_init_resume<ev64.value>, grid, block, 0, as_stream(stream), batch, n_events,
                               static_cast<const Ev *>(ev_planes), t_start, n_avg, init, t_init, ready, state,
                               (int32_t)(resume != 0));
        },
        (flags & PEKF_EV_F64_EVENTS) != 0);
    return launched("k_frontend_init_resume");
}
