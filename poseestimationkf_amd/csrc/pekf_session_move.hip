// pekf_session_move.hip -- a live phone moves (pekf_session_export_dev, pekf_session_import_dev,
// pekf_session_columns_bytes): k_session_recycle's counterpart (pekf_session_recycle.hip).  Where that kernel
// writes a listed column's fresh form, these copy its live form out of a session into a packed buffer and from a
// packed buffer into a session -- the same one or another, of another batch, on another device once the pack's
// bytes have been copied there.  A file of its own, so that the session kernels' objects and listings hold the
// kernels they held.
//
// The reference has nothing to compare: it serves one client per process (KFS/Server.cpp:58, :93), so a phone
// never changes its place.  A column of a batch does: a sparse session is gathered into a smaller one, a phone
// goes to another shard, or is forked.  Everything a column holds is lane-minor and private, and each piece's
// layout has one owner, read here and not restated:
//   the filter (LiveState<true>, pekf_live.hpp): its kPlanes planes, the join mark among them; X, P, refs;
//   phase 2 (InitState, pekf_phase2.hpp): its kPlanes planes; t_start, init, t_init, ready;
//   phase 1 (MagcalState, pekf_magcal.hpp): the two header planes and the 3 n_cal sample planes, through
//     MagcalState::sample on both sides; cal, fit, status.
//
// The pack (PackLayout below) is one buffer of lane-minor planes over the n listed columns, [plane][n], 16 B per
// entry, so the packed side of every access is contiguous per wave; the session side is scattered, as a column
// list implies.  Going through it makes source and destination independent: nothing is ever copied in place.
// Pure data movement, 0.7 KB per listed column and 32 + 24 n_cal + 160 B more with phase 1; nothing here is tuned.
#include "pekf_live.hpp"
#include "pekf_magcal.hpp"
#include "pekf_phase2.hpp"

namespace pekf {

constexpr int kMoveBlock = 256;

// Where the pack's planes are, in 16 B entries per listed column from the pack's start.  The sections follow
// the pack's flags and n_cal, not the groups a call is handed, so a pack has one layout for its whole life:
//   flags == PEKF_EV_F64_EVENTS (a joining session's): the filter -- LiveState's planes, X (2), P (8), refs (3) --
//     then phase 2 -- InitState's planes, {t_start, t_init} (1), init (3), {ready} (1);
//   n_cal != 0: phase 1 -- a MagcalState of batch n (MagcalState::bytes_per_phone(n_cal) per column: the header
//     planes, the sample planes of 8 B per entry), then cal (6), fit (3), {status} (1).
struct PackLayout {
    static constexpr int kLive = 0, kX = kLive + LiveState<true>::kPlanes, kP = kX + 2, kRefs = kP + 8;
    static constexpr int kInit = kRefs + 3, kTimes = kInit + InitState::kPlanes, kInitOut = kTimes + 1;
    static constexpr int kReady = kInitOut + 3, kSessionPlanes = kReady + 1;  // filter + phase 2
    static constexpr int kCal = 0, kFit = kCal + 6, kStatus = kFit + 3, kPhase1OutPlanes = kStatus + 1;

    int64_t n;
    int64_t magcal;   // byte offset of the MagcalState of batch n
    int64_t p1_out;   // byte offset of the phase-1 outputs' planes
    int64_t bytes;
    __host__ __device__ PackLayout(int64_t n_cols, int n_cal, bool session) : n(n_cols) {
        magcal = session ? 16 * (int64_t)kSessionPlanes * n : 0;
        p1_out = magcal + (n_cal ? n * MagcalState::bytes_per_phone(n_cal) : 0);
        bytes = p1_out + (n_cal ? 16 * (int64_t)kPhase1OutPlanes * n : 0);
    }
};

struct MoveArgs {
    int64_t batch, n_cols;
    const int32_t *cols;
    // the filter
    void *live_state;
    double *X, *P, *refs;
    // phase 2
    void *init_state;
    int64_t *t_start;
    double *init;
    int64_t *t_init;
    int32_t *ready;
    // phase 1
    void *magcal_state;
    int n_cal;
    double *cal, *fit;
    int32_t *status;
    // the pack and its sections
    void *pack;
    int64_t magcal_off, p1_out_off;
};

// one 16 B plane entry between the session and the pack
template <bool EXPORT>
__device__ __forceinline__ void move_plane(double2 *session, double2 *pack) {
    if constexpr (EXPORT)
        *pack = *session;
    else
        *session = *pack;
}
// 2 * PLANES doubles of an output array (8-byte aligned, as the session kernels take them) and their planes
template <bool EXPORT, int PLANES>
__device__ __forceinline__ void move_doubles(double *session, void *pack, int64_t n, int64_t i, int plane0) {
#pragma unroll
    for (int pl = 0; pl < PLANES; ++pl) {
        double2 *p = state_plane(pack, n, i, plane0 + pl);
        if constexpr (EXPORT) {
            *p = make_double2(session[2 * pl], session[2 * pl + 1]);
        } else {
            const double2 v = *p;
            session[2 * pl] = v.x;
            session[2 * pl + 1] = v.y;
        }
    }
}

// One lane per listed column, looping over the planes.  EXPORT: the session is read and the pack written;
// otherwise the pack is read and the session written.  A lane whose index is outside [0, batch) reads and
// writes nothing.
template <bool EXPORT>
__global__ __launch_bounds__(kMoveBlock) void k_session_move(MoveArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kMoveBlock + threadIdx.x;
    if (i >= a.n_cols) return;
    const int64_t b = a.cols[i];
    if (b < 0 || b >= a.batch) return;
    const int64_t n = a.n_cols;
    using L = PackLayout;

    if (a.live_state) {  // uniform, as every test of a group's pointer below
#pragma unroll
        for (int pl = 0; pl < LiveState<true>::kPlanes; ++pl)
            move_plane<EXPORT>(state_plane(a.live_state, a.batch, b, pl), state_plane(a.pack, n, i, L::kLive + pl));
        move_doubles<EXPORT, 2>(a.X + 4 * b, a.pack, n, i, L::kX);
        move_doubles<EXPORT, 8>(a.P + 16 * b, a.pack, n, i, L::kP);
        move_doubles<EXPORT, 3>(a.refs + 6 * b, a.pack, n, i, L::kRefs);
    }

    if (a.init_state) {
#pragma unroll
        for (int pl = 0; pl < InitState::kPlanes; ++pl)
            move_plane<EXPORT>(state_plane(a.init_state, a.batch, b, pl), state_plane(a.pack, n, i, L::kInit + pl));
        move_doubles<EXPORT, 3>(a.init + 6 * b, a.pack, n, i, L::kInitOut);
        double2 *times = state_plane(a.pack, n, i, L::kTimes), *rdy = state_plane(a.pack, n, i, L::kReady);
        if constexpr (EXPORT) {
            *times = make_double2(__longlong_as_double(a.t_start[b]), __longlong_as_double(a.t_init[b]));
            *rdy = make_double2(__hiloint2double(0, a.ready[b]), 0.0);
        } else {
            const double2 t = *times;
            a.t_start[b] = __double_as_longlong(t.x);
            a.t_init[b] = __double_as_longlong(t.y);
            a.ready[b] = __double2loint(rdy->x);
        }
    }

    if (a.magcal_state) {
        void *pm = static_cast<unsigned char *>(a.pack) + a.magcal_off;   // a MagcalState of batch n
        void *po = static_cast<unsigned char *>(a.pack) + a.p1_out_off;
#pragma unroll
        for (int pl = 0; pl < MagcalState::kHeadPlanes; ++pl)
            move_plane<EXPORT>(state_plane(a.magcal_state, a.batch, b, pl), state_plane(pm, n, i, pl));
        for (int k = 0; k < a.n_cal; ++k) {  // uniform: a launch argument
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double *s = MagcalState::sample(a.magcal_state, a.batch, b, k, c);
                double *p = MagcalState::sample(pm, n, i, k, c);
                if constexpr (EXPORT)
                    *p = *s;
                else
                    *s = *p;
            }
        }
        move_doubles<EXPORT, 6>(a.cal + 12 * b, po, n, i, L::kCal);
        move_doubles<EXPORT, 3>(a.fit + 6 * b, po, n, i, L::kFit);
        double2 *st = state_plane(po, n, i, L::kStatus);
        if constexpr (EXPORT)
            *st = make_double2(__hiloint2double(0, a.status[b]), 0.0);
        else
            a.status[b] = __double2loint(st->x);
    }
}

}  // namespace pekf

using namespace pekf;

static bool aligned16(const void *p) { return (uintptr_t)p % 16 == 0; }
static bool pack_flags_ok(uint32_t flags) { return flags == 0 || flags == PEKF_EV_F64_EVENTS; }

static_assert(sizeof(long long) == sizeof(int64_t), "pekf_session_columns_bytes returns 64 bits");
extern "C" long long int pekf_session_columns_bytes(int64_t n_cols, int n_cal, uint32_t flags) {
    if (n_cols < 0 || n_cols >= ((int64_t)1 << 28) || !pack_flags_ok(flags)) return -1;
    if (n_cal != 0 && (n_cal < 6 || n_cal >= (1 << 30))) return -1;
    return PackLayout(n_cols, n_cal, flags == PEKF_EV_F64_EVENTS).bytes;
}

// The checks and the launch both entries share (the session's pointers const or not is the entries' business)
template <bool EXPORT>
static int session_move(int64_t batch, int64_t n_cols, const int32_t *cols, uint32_t flags, void *live_state, double *X,
                        double *P, double *refs, void *init_state, int64_t *t_start, double *init, int64_t *t_init,
                        int32_t *ready, void *magcal_state, int n_cal, double *cal, double *fit, int32_t *status,
                        void *pack, void *stream) {
    PEKF_CHECK_ARG(batch >= 0 && n_cols >= 0, "negative size");
    PEKF_CHECK_ARG(batch < ((int64_t)1 << 28), "batch must be < 2^28 phones per launch");
    PEKF_CHECK_ARG(aligned16(live_state), "live_state must be a 16-byte aligned pointer");
    PEKF_CHECK_ARG(aligned16(init_state), "init_state must be a 16-byte aligned pointer");
    PEKF_CHECK_ARG(aligned16(magcal_state), "magcal_state must be a 16-byte aligned pointer");
    PEKF_CHECK_ARG(aligned16(pack), "pack must be a 16-byte aligned pointer");
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
    PEKF_CHECK_ARG(any_1 || n_cal == 0, "n_cal without the phase-1 group must be 0 (it sizes the pack)");
    PEKF_CHECK_ARG(pack_flags_ok(flags) && (!(any_f || any_2) || flags == PEKF_EV_F64_EVENTS),
                   "the filter and phase-2 groups are a joining session's (flags must be PEKF_EV_F64_EVENTS, as "
                   "pekf_live_join_dev; 0 for a pack of the phase-1 group alone)");
    if (n_cols == 0 || batch == 0 || !(any_f || any_2 || any_1)) return PEKF_OK;
    PEKF_CHECK_ARG(cols && pack, "null pointer");
    PEKF_CHECK_ARG(n_cols <= batch, "cols lists distinct columns: n_cols must be <= batch");
    const PackLayout lay(n_cols, n_cal, flags == PEKF_EV_F64_EVENTS);
    const MoveArgs a = {batch, n_cols, cols, live_state, X, P, refs, init_state, t_start, init, t_init, ready,
                        magcal_state, n_cal, cal, fit, status, pack, lay.magcal, lay.p1_out};
    hipLaunchKernelGGL(k_session_move<EXPORT>, dim3(grid_for(n_cols, kMoveBlock)), dim3(kMoveBlock), 0,
                       as_stream(stream), a);
    return launched(EXPORT ? "k_session_move (export)" : "k_session_move (import)");
}

extern "C" int pekf_session_export_dev(int64_t batch, int64_t n_cols, const int32_t *cols, uint32_t flags,
                                       const void *live_state, const double *X, const double *P, const double *refs,
                                       const void *init_state, const int64_t *t_start, const double *init,
                                       const int64_t *t_init, const int32_t *ready, const void *magcal_state,
                                       int n_cal, const double *cal, const double *fit, const int32_t *status,
                                       void *pack, void *stream) {
    // (the kernel's EXPORT form reads the session and writes the pack alone)
    return session_move<true>(batch, n_cols, cols, flags, const_cast<void *>(live_state), const_cast<double *>(X),
                              const_cast<double *>(P), const_cast<double *>(refs), const_cast<void *>(init_state),
                              const_cast<int64_t *>(t_start), const_cast<double *>(init),
                              const_cast<int64_t *>(t_init), const_cast<int32_t *>(ready),
                              const_cast<void *>(magcal_state), n_cal, const_cast<double *>(cal),
                              const_cast<double *>(fit), const_cast<int32_t *>(status), pack, stream);
}

extern "C" int pekf_session_import_dev(int64_t batch, int64_t n_cols, const int32_t *cols, uint32_t flags,
                                       void *live_state, double *X, double *P, double *refs, void *init_state,
                                       int64_t *t_start, double *init, int64_t *t_init, int32_t *ready,
                                       void *magcal_state, int n_cal, double *cal, double *fit, int32_t *status,
                                       const void *pack, void *stream) {
    return session_move<false>(batch, n_cols, cols, flags, live_state, X, P, refs, init_state, t_start, init, t_init,
                               ready, magcal_state, n_cal, cal, fit, status, const_cast<void *>(pack), stream);
}
