// pekf_live.hpp -- k_live, the fused front-end + filter kernel, and its record queue (see pekf_live.hip,
// which instantiates the kernels without trajectory output; pekf_live_traj.hip instantiates their TRAJ twins,
// pekf_live_resume.hip the resumable kernels of a session fed in chunks, pekf_live_join.hip those whose filters
// join the session one by one, pekf_live_rec.hip those that hand out their records).  The host side every pekf_live_* entry shares closes the file: LiveCall (the
// entries' common arguments), their checks, and the one launcher, launch_k_live<TRAJ, RESUME, JOIN>.
#pragma once
#include "pekf_phase3.hpp"
#include "pekf_step.hpp"

namespace pekf {

// Tuned on the box (scripts/ab_live.sh, profiles/r2/live/): the kernel is register-bound -- front-end
// state, filter state and a filter step's temporaries -- so the record queue lives in LDS and the
// launch is held to 2 waves per SIMD (252 registers) with a 3-event ring: 5.5 ms at 1M filters x
// 1,024 events, against 8.7 ms for 6 events and the queue in registers at 1 wave/SIMD.  Queueing the
// records' raw inputs instead (emit moved into the filter step, 104 B per slot, 3 deep) was slower:
// 5.9 ms (profiles/r2/live/variants/raw_queue.log).
#ifndef PEKF_LIVE_RING
#define PEKF_LIVE_RING 3  // event rows in flight per lane; a filter step may run after each block of them
#endif
#ifndef PEKF_LIVE_RING64
#define PEKF_LIVE_RING64 3  // the same for FP64 events (32 B each)
#endif
#ifndef PEKF_LIVE_NTL
#define PEKF_LIVE_NTL 1  // non-temporal event loads: each event is read once (-1.4 %, profiles/r4/ntload/)
#endif
#ifndef PEKF_LIVE_QUEUE
#define PEKF_LIVE_QUEUE 6  // records a lane can hold (48 B of LDS each: the 40 B record + its escaped dt)
#endif
#ifndef PEKF_LIVE_QUEUE64
#define PEKF_LIVE_QUEUE64 5  // the same with FP64 acc / mag (64 B each): 20 KB of LDS per wave, all of it
#endif
#ifndef PEKF_LIVE_QUEUE_EV64
#define PEKF_LIVE_QUEUE_EV64 4  // FP64 events: all-FP64 records (80 B each), 20 KB of LDS per wave
#endif
#ifndef PEKF_LIVE_QUORUM
#define PEKF_LIVE_QUORUM 56  // lanes of 64 with a queued record that trigger a filter step
#endif
#ifndef PEKF_LIVE_EV64_WAVES
#define PEKF_LIVE_EV64_WAVES 2
#endif
#ifndef PEKF_LIVE_TRAJ_LATE
// 0: a TRAJ kernel forms each trajectory row in the filter step.  1: the step stores the raw reference-basis
// X and each lane converts its own rows in place after the event loop (the same function on the same
// doubles, so the same bits): 26-32 spilled VGPRs instead of 58, but each row written twice and read once --
// 7.8 against 6.3 ms at 1M filters x 1,024 events, same-box A B B A (profiles/r12/live_traj/README.md).
#define PEKF_LIVE_TRAJ_LATE 0
#endif

// A lane's records waiting for the wave's next filter step, oldest first: a ring of Q slots per lane in
// LDS, [slot][lane] so that a wave's accesses fall in distinct banks whatever slot each lane is at.  A
// push or pop is a few address operations and three to five 16-byte LDS accesses.  (Held in registers --
// slots as separate variables, a push selecting its slot -- the queue cost 40 selects per push and
// registers the kernel does not have: profiles/r2/live/variants/live_ab*.log.)
//
// The ring is RecordQueue; what a slot holds is one of three layouts, one per record form of
// Phase3T::finish (In: the form pushed).  A layout states its LDS planes and their bytes, how a record is
// stored, how a slot is loaded and becomes gy / acc / mag, and where a dt that does not fit the f32 forms'
// dt word (PEKF_DT_ESCAPE, a pause of 2^31 ns or more) is kept: keep_dt on the push of such a record,
// take_dt on every pop (the record's dt in ns; has: a record was queued).

// The f32 stream record (PEKF_EV_F32_RECORDS: what pekf_frontend_dev writes), 48 B per slot: the 40 B
// record and an escaped-dt plane dt[slot][lane], written and read only for an escaped record; 6 slots
// are 18 KB per wave.
template <int Q>
struct SlotsF32 {
    using In = Rec;
    using Slot = Rec;
    static constexpr size_t kBytes = (sizeof(float4) * 2 + sizeof(float2) + sizeof(double)) * Q * kRunBlock;
    float4 (*gd)[kRunBlock];
    float4 (*am)[kRunBlock];
    float2 (*my)[kRunBlock];
    double (*dt)[kRunBlock];
    __device__ __forceinline__ void bind(unsigned char *lds) {
        gd = reinterpret_cast<float4(*)[kRunBlock]>(lds);
        am = reinterpret_cast<float4(*)[kRunBlock]>(lds + sizeof(float4) * Q * kRunBlock);
        dt = reinterpret_cast<double(*)[kRunBlock]>(lds + 2 * sizeof(float4) * Q * kRunBlock);
        my = reinterpret_cast<float2(*)[kRunBlock]>(lds + (2 * sizeof(float4) + sizeof(double)) * Q * kRunBlock);
    }
    __device__ __forceinline__ void store(int slot, const In &r) {
        gd[slot][threadIdx.x] = r.gd;
        am[slot][threadIdx.x] = r.am;
        my[slot][threadIdx.x] = r.my;
    }
    __device__ __forceinline__ Slot load(int slot) const {
        return {gd[slot][threadIdx.x], am[slot][threadIdx.x], my[slot][threadIdx.x]};
    }
    static __device__ __forceinline__ void unpack(const Slot &r, double *gy, double *acc, double *mag) {
        gy[0] = r.gd.x; gy[1] = r.gd.y; gy[2] = r.gd.z;
        acc[0] = r.am.x; acc[1] = r.am.y; acc[2] = r.am.z;
        mag[0] = r.am.w; mag[1] = r.my.x; mag[2] = r.my.y;
    }
    __device__ __forceinline__ bool esc_queued() const { return false; }  // escaped dts live in the dt plane
    __device__ __forceinline__ void keep_dt(int slot, double dtv) { dt[slot][threadIdx.x] = dtv; }
    __device__ __forceinline__ double take_dt(int slot, const Slot &r, bool) {
        const uint32_t word = __float_as_uint(r.gd.w) & PEKF_DT_MASK;
        double dtv = (double)word;
        if (word == PEKF_DT_ESCAPE) dtv = dt[slot][threadIdx.x];
        return dtv;
    }
};

// The f32 gyro / dt word with FP64 acc / mag: what the server's filter receives (KFS/KalmanFilter.cpp:279-303
// hands the double low-pass outputs to Prediction / Correction), not the f32 stream record.  Per slot the
// gyro / dt word (16 B) and acc and mag as three double2 planes (48 B): 5 slots x 64 B x 64 lanes is
// 20 KB per wave, exactly the CU's 160 KB at 2 waves per SIMD, so there is no room for an escaped-dt
// plane.  An escaped record keeps its float64 dt in a register instead (esc_dt), one per lane: k_live
// steps a wave while any lane still has such a record queued (want_step) and completes at most one
// record per lane and block (its kPush == 1 static_assert), so a lane never holds two (escapes are pauses
// of 2.1 s or more: rare, and cheap to drain for).
template <int Q>
struct SlotsLpf {
    using In = RecLpf;
    struct Slot {
        float4 gd;
        double2 v[3];
    };
    static constexpr size_t kBytes = (sizeof(float4) + 3 * sizeof(double2)) * Q * kRunBlock;
    float4 (*gd)[kRunBlock];
    double2 (*am)[3][kRunBlock];  // {acc.x, acc.y}, {acc.z, mag.x}, {mag.y, mag.z}
    double esc_dt = __builtin_nan("");  // the queued escaped record's dt (NaN: none queued)
    __device__ __forceinline__ void bind(unsigned char *lds) {
        am = reinterpret_cast<double2(*)[3][kRunBlock]>(lds);
        gd = reinterpret_cast<float4(*)[kRunBlock]>(lds + 3 * sizeof(double2) * Q * kRunBlock);
    }
    __device__ __forceinline__ void store(int slot, const In &r) {
        gd[slot][threadIdx.x] = r.gd;
        am[slot][0][threadIdx.x] = make_double2(r.acc.x, r.acc.y);
        am[slot][1][threadIdx.x] = make_double2(r.acc.z, r.mag.x);
        am[slot][2][threadIdx.x] = make_double2(r.mag.y, r.mag.z);
    }
    __device__ __forceinline__ Slot load(int slot) const {
        return {gd[slot][threadIdx.x], {am[slot][0][threadIdx.x], am[slot][1][threadIdx.x], am[slot][2][threadIdx.x]}};
    }
    static __device__ __forceinline__ void unpack(const Slot &r, double *gy, double *acc, double *mag) {
        gy[0] = r.gd.x; gy[1] = r.gd.y; gy[2] = r.gd.z;
        acc[0] = r.v[0].x; acc[1] = r.v[0].y; acc[2] = r.v[1].x;
        mag[0] = r.v[1].y; mag[1] = r.v[2].x; mag[2] = r.v[2].y;
    }
    // a lane has an escaped record queued (k_live then steps until it is applied)
    __device__ __forceinline__ bool esc_queued() const { return esc_dt == esc_dt; }
    __device__ __forceinline__ void keep_dt(int, double dtv) { esc_dt = dtv; }
    __device__ __forceinline__ double take_dt(int, const Slot &r, bool has) {
        const uint32_t word = __float_as_uint(r.gd.w) & PEKF_DT_MASK;
        double dtv = (double)word;
        if (has && word == PEKF_DT_ESCAPE) {
            dtv = esc_dt;
            esc_dt = __builtin_nan("");
        }
        return dtv;
    }
};

// The all-FP64 record of FP64-event launches: gyro and dt too, as the server's filter gets them -- the dt
// any float64, so there is no escape and nothing to keep -- 80 B per slot as five double2 planes
// [slot][lane] (16 B per lane and plane: conflict-free ds_*_b128), 4 deep = 20 KB per wave, the CU's
// 160 KB at 2 waves per SIMD.
template <int Q>
struct SlotsF64 {
    using In = Rec64;
    struct Slot {
        double2 v[5];
    };
    static constexpr size_t kBytes = 5 * sizeof(double2) * Q * kRunBlock;
    double2 (*v)[5][kRunBlock];  // {gx, gy}, {gz, dt}, {ax, ay}, {az, mx}, {my, mz}
    __device__ __forceinline__ void bind(unsigned char *lds) { v = reinterpret_cast<double2(*)[5][kRunBlock]>(lds); }
    __device__ __forceinline__ void store(int slot, const In &r) {
        v[slot][0][threadIdx.x] = make_double2(r.gd.x, r.gd.y);
        v[slot][1][threadIdx.x] = make_double2(r.gd.z, r.gd.w);
        v[slot][2][threadIdx.x] = make_double2(r.am.x, r.am.y);
        v[slot][3][threadIdx.x] = make_double2(r.am.z, r.am.w);
        v[slot][4][threadIdx.x] = r.my;
    }
    __device__ __forceinline__ Slot load(int slot) const {
        Slot r;
#pragma unroll
        for (int k = 0; k < 5; ++k) r.v[k] = v[slot][k][threadIdx.x];
        return r;
    }
    static __device__ __forceinline__ void unpack(const Slot &r, double *gy, double *acc, double *mag) {
        gy[0] = r.v[0].x; gy[1] = r.v[0].y; gy[2] = r.v[1].x;
        acc[0] = r.v[2].x; acc[1] = r.v[2].y; acc[2] = r.v[3].x;
        mag[0] = r.v[3].y; mag[1] = r.v[4].x; mag[2] = r.v[4].y;
    }
    __device__ __forceinline__ bool esc_queued() const { return false; }
    __device__ __forceinline__ void keep_dt(int, double) {}
    __device__ __forceinline__ double take_dt(int, const Slot &r, bool) { return r.v[1].y; }
};

// The ring over a layout's Q slots: head, the n records queued from it, the tail a push fills
template <template <int> class Slots, int Q>
struct RecordQueue : Slots<Q> {
    int head = 0, n = 0;
    __device__ __forceinline__ int tail() const { return head + n < Q ? head + n : head + n - Q; }
    // the slot popped last: its record stays there until a later push
    __device__ __forceinline__ int last() const { return head == 0 ? Q - 1 : head - 1; }
    __device__ __forceinline__ void push(const typename Slots<Q>::In &r, bool esc, double dtv) {
        const int slot = tail();
        this->store(slot, r);
        if (esc) this->keep_dt(slot, dtv);
        ++n;
    }
    // the oldest record and its dt in ns
    __device__ __forceinline__ typename Slots<Q>::Slot pop(double &dtv) {
        const typename Slots<Q>::Slot r = this->load(head);
        dtv = this->take_dt(head, r, n > 0);
        if (n > 0) {
            head = head + 1 < Q ? head + 1 : 0;
            --n;
        }
        return r;
    }
    // the popped record's acc / mag again
    __device__ __forceinline__ void reload(double *a, double *m) const {
        double gy[3];
        Slots<Q>::unpack(this->load(last()), gy, a, m);
    }
};

// A resumable launch's session state (k_live<..., RESUME>): what a lane holds between two event blocks, so that
// the next launch on the same filters' next events continues as one launch over all of them would.  The
// front-end: every member Phase3T::start sets but the phase-2 means and alpha / beta (remade from init and
// alpha) and pend / p (nothing is pending after a whole block, and a launch ends on one).  The filter as the loop
// holds it: the unnormalised reference-basis x, the ten entries of N, and `total`, the records the filter has
// applied since the session began (the first of them alone takes the eager step).  The record queue is empty at
// a launch's end, so nothing of it is carried.
//
// One device buffer of filter-minor planes of 16 B per lane, [plane][batch]: a wave's load or store of a plane
// is one contiguous 1 KB access.  Two doubles pair up in a plane, four f32 samples in one; the five flags and
// `total` share the last double's plane.  f32 events: 27 doubles + {flags, total} in 14 planes and the 15 f32
// sample words in 4, 288 B per filter.  FP64 events: 41 doubles + {flags, total} in 21 planes, 336 B (their
// running clock t is never read: FP64 events carry their times).  Read once before the event loop, written
// once after it.
template <bool EV64>
struct LiveState {
    using Fe = Phase3T<std::conditional_t<EV64, V3, F3>>;
    static constexpr int kDoubles = EV64 ? 42 : 28;                 // the last one holds {flags, total}
    static constexpr int kPlanes = kDoubles / 2 + (EV64 ? 0 : 4);   // f32 events: 4 float4 planes of samples
    static constexpr int kBytes = 16 * kPlanes;                     // per filter

    template <bool LOAD, typename T>
    static __device__ __forceinline__ void mv(T &member, double &word) {
        if constexpr (LOAD)
            member = word;
        else
            word = member;
    }
    // the doubles in their order in the planes, to (LOAD = false) or from d
    template <bool LOAD>
    static __device__ __forceinline__ void doubles(Fe &fe, double *x, Sym4T<double> &N, double (&d)[kDoubles]) {
        int k = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) mv<LOAD>(x[i], d[k++]);
        mv<LOAD>(N.a00, d[k++]); mv<LOAD>(N.a01, d[k++]); mv<LOAD>(N.a02, d[k++]); mv<LOAD>(N.a03, d[k++]);
        mv<LOAD>(N.a11, d[k++]); mv<LOAD>(N.a12, d[k++]); mv<LOAD>(N.a13, d[k++]); mv<LOAD>(N.a22, d[k++]);
        mv<LOAD>(N.a23, d[k++]); mv<LOAD>(N.a33, d[k++]);
        mv<LOAD>(fe.lpf_acc.x, d[k++]); mv<LOAD>(fe.lpf_acc.y, d[k++]); mv<LOAD>(fe.lpf_acc.z, d[k++]);
        mv<LOAD>(fe.lpf_mag.x, d[k++]); mv<LOAD>(fe.lpf_mag.y, d[k++]); mv<LOAD>(fe.lpf_mag.z, d[k++]);
        mv<LOAD>(fe.t_acc0, d[k++]); mv<LOAD>(fe.t_mag0, d[k++]); mv<LOAD>(fe.prev_t, d[k++]);
        mv<LOAD>(fe.t_acc1, d[k++]); mv<LOAD>(fe.t_mag1, d[k++]); mv<LOAD>(fe.t_gyro, d[k++]);
        if constexpr (EV64) {
            mv<LOAD>(fe.acc0.x, d[k++]); mv<LOAD>(fe.acc0.y, d[k++]); mv<LOAD>(fe.acc0.z, d[k++]);
            mv<LOAD>(fe.mag0.x, d[k++]); mv<LOAD>(fe.mag0.y, d[k++]); mv<LOAD>(fe.mag0.z, d[k++]);
            mv<LOAD>(fe.acc1.x, d[k++]); mv<LOAD>(fe.acc1.y, d[k++]); mv<LOAD>(fe.acc1.z, d[k++]);
            mv<LOAD>(fe.mag1.x, d[k++]); mv<LOAD>(fe.mag1.y, d[k++]); mv<LOAD>(fe.mag1.z, d[k++]);
            mv<LOAD>(fe.gyro.x, d[k++]); mv<LOAD>(fe.gyro.y, d[k++]); mv<LOAD>(fe.gyro.z, d[k++]);
        } else {
            mv<LOAD>(fe.t, d[k++]);
        }
    }
    static __device__ __forceinline__ void load(void *state, int64_t batch, int64_t b, Fe &fe, double *x,
                                                Sym4T<double> &N, int32_t &total) {
        double d[kDoubles];
#pragma unroll
        for (int p = 0; p < kDoubles / 2; ++p) {
            const double2 v = *state_plane(state, batch, b, p);
            d[2 * p] = v.x;
            d[2 * p + 1] = v.y;
        }
        doubles<true>(fe, x, N, d);
        const uint32_t flags = (uint32_t)__double2loint(d[kDoubles - 1]);
        total = __double2hiint(d[kDoubles - 1]);
        fe.acc0_mean = flags & 1u; fe.mag0_mean = flags & 2u;
        fe.gyro_set = flags & 4u; fe.acc1_set = flags & 8u; fe.mag1_set = flags & 16u;
        if constexpr (!EV64) {
            float4 s[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) s[p] = *reinterpret_cast<const float4 *>(state_plane(state, batch, b, kDoubles / 2 + p));
            fe.acc0 = {s[0].x, s[0].y, s[0].z}; fe.mag0 = {s[0].w, s[1].x, s[1].y};
            fe.acc1 = {s[1].z, s[1].w, s[2].x}; fe.mag1 = {s[2].y, s[2].z, s[2].w};
            fe.gyro = {s[3].x, s[3].y, s[3].z};
        }
    }
    // the flag word's bit 5 (k_live<..., JOIN>): this lane has joined the session -- its state is to be resumed
    static constexpr uint32_t kJoined = 32u;
    static __device__ __forceinline__ bool joined(void *state, int64_t batch, int64_t b) {
        return ((uint32_t)__double2loint(state_plane(state, batch, b, kDoubles / 2 - 1)->y) & kJoined) != 0;
    }
    static __device__ __forceinline__ void store(void *state, int64_t batch, int64_t b, Fe &fe, double *x,
                                                 Sym4T<double> &N, int32_t total, uint32_t mark = 0u) {
        double d[kDoubles];
        doubles<false>(fe, x, N, d);
        const uint32_t flags = (fe.acc0_mean ? 1u : 0u) | (fe.mag0_mean ? 2u : 0u) | (fe.gyro_set ? 4u : 0u) |
                               (fe.acc1_set ? 8u : 0u) | (fe.mag1_set ? 16u : 0u) | mark;
        d[kDoubles - 1] = __hiloint2double(total, (int)flags);
#pragma unroll
        for (int p = 0; p < kDoubles / 2; ++p) *state_plane(state, batch, b, p) = make_double2(d[2 * p], d[2 * p + 1]);
        if constexpr (!EV64) {
            const float4 s[4] = {make_float4(fe.acc0.x, fe.acc0.y, fe.acc0.z, fe.mag0.x),
                                 make_float4(fe.mag0.y, fe.mag0.z, fe.acc1.x, fe.acc1.y),
                                 make_float4(fe.acc1.z, fe.mag1.x, fe.mag1.y, fe.mag1.z),
                                 make_float4(fe.gyro.x, fe.gyro.y, fe.gyro.z, 0.f)};
#pragma unroll
            for (int p = 0; p < 4; ++p) *reinterpret_cast<float4 *>(state_plane(state, batch, b, kDoubles / 2 + p)) = s[p];
        }
    }
};

// Where a REC kernel (k_live<..., REC>) leaves the records it applies: three filter-minor planes [row][batch] in
// pekf_run_rec64_dev's layout (RecordWindow64's) -- gd double4 {gx, gy, gz, dt_ns}, am double4 {ax, ay, az, mx},
// my double2 {my, mz}.  Without REC the argument is empty, as NoiseR is without a plane (pekf_step.hpp), so the
// other kernels' argument block, and with it their code, is what it was.
struct NoRecArg {};
struct RecPlanesArg {
    double4 *gd, *am;
    double2 *my;
};
template <bool REC>
using RecPlanes = std::conditional_t<REC, RecPlanesArg, NoRecArg>;

// TE: the event planes may hold time events (Phase3::event).  R64: records keep their FP64 acc / mag
// (SlotsLpf); otherwise they are the f32 stream records pekf_frontend_dev writes (SlotsF32).
// EV64: FP64 events (PEKF_EV_F64_EVENTS, double4 planes: the server's own sample values), records all
// FP64 (SlotsF64); TE and R64 do not apply.
// TRAJ: a pose per record (the server's X_k, Parser::ExecuteKalmanFilter, KFS/Parser.cpp:248-267): the
// lane's r-th record of the launch (r < traj_rows) leaves its world-basis unit X in traj[r][b] (4 doubles,
// formed by ref_to_world as k_run's trajectory row and the launch's final X are) and, with traj_dt, the dt
// in ns it was applied with in traj_dt[r][b].  The row is the lane's own record index, not the wave's step
// number: lanes complete records at different events, so a wave's 64 stores fall in up to 64 rows.  Nothing
// else is written (rows >= counts[b], every row of a filter that is not ready or has no record).  The
// kernels without TRAJ read none of the three arguments.
// RESUME: a session fed in several launches (pekf_live_resume_dev).  The lane's session state (LiveState) is
// stored in `state` after the event loop -- the raw x and N, before from_ref_basis touches them -- and, with
// resume != 0, loaded from it before the loop in place of the fresh start (fe.start, load_state and
// enter_ref_basis's rotation; Wr depends on the references alone and is made from init as ever).  The first
// record of a launch takes the eager form only if the filter has applied none in the whole session, so every
// record is applied by the call the single launch makes for it and any cutting of a session's events into
// launches gives the single launch's bits.  X / P are written, and counts[b] and the trajectory rows count, per
// launch.  The kernels without RESUME read neither argument.
// JOIN (with RESUME, FP64 events: pekf_live_join_dev): each lane joins the session by itself.  Not `resume` but
// the lane's own mark in its state's flag word (LiveState::kJoined; the caller zeroes the state before the first
// launch) says whether it continues from the state or starts fresh as resume == 0 does, from this launch's init /
// t_init and X / P.  A lane is marked, and its state stored, at the end of a launch in which it was ready and
// its column held a message; until then nothing of it is kept -- null rows move no state, so the fresh start at
// the launch with its first message is the one launch that walked the null rows before it.
// NOISE (with RESUME; pekf_live_resume_noise.hip, pekf_live_join_noise.hip): per-filter noise, the lane's own q
// and r from the {q, r} plane (NoiseQ, pekf_step.hpp) in place of the launch's.  The session state holds the
// covariance as N, P = rI + sqrt(2) r D N D, so a lane's r must stay what it was for as long as its session lasts.
// REC (with TRAJ and RESUME; pekf_live_rec.hip, pekf_live_rec_noise.hip): the record each pose came from, the
// server's log lines gyro / Acc_1 / Mag_1 and the dt between its T lines (KalmanFilter::WriteTextFile).  The lane's
// r-th record of the launch (r < traj_rows, the pose's row) leaves the doubles handed to ekf_record_step in
// rec.gd / rec.am / rec.my [r][b] -- an f32-event record's f32 gyro widened, its dt the double take_dt returned
// (an escaped one too); an FP64-event record's slot as it is -- stored before the step, so nothing more is live
// across it: five 16-byte stores, into the lane's own row as the pose's are.  Nothing else is written.
template <bool TE, bool R64, bool EV64 = false, bool TRAJ = false, bool RESUME = false, bool JOIN = false,
          bool NOISE = false, bool REC = false>
__global__ __launch_bounds__(kRunBlock) __attribute__((amdgpu_waves_per_eu(EV64 ? PEKF_LIVE_EV64_WAVES : 2))) void k_live(
    int64_t batch, int64_t n_events, const std::conditional_t<EV64, double4, float4> *__restrict__ ev,
    const double *__restrict__ init, const int64_t *__restrict__ t_init, double alpha, NoiseQ<NOISE> q_arg,
    NoiseR<NOISE> r_arg,
    double *__restrict__ Xio, double *__restrict__ Pio, int32_t *__restrict__ counts, double *__restrict__ refs,
    double *__restrict__ traj, double *__restrict__ traj_dt, int32_t traj_rows, void *__restrict__ state,
    int32_t resume, RecPlanes<REC> rec) {
    using EvT = std::conditional_t<EV64, double4, float4>;
    constexpr int kRing = EV64 ? PEKF_LIVE_RING64 : PEKF_LIVE_RING, kFlush = 3, kQuorum = PEKF_LIVE_QUORUM;
    constexpr int kQueue = EV64 ? PEKF_LIVE_QUEUE_EV64 : R64 ? PEKF_LIVE_QUEUE64 : PEKF_LIVE_QUEUE;
    constexpr int kPush = kRing / kFlush;  // records a lane can complete within one block
    static_assert(kRing % kFlush == 0, "the ring depth must be a multiple of the emit period");
    static_assert(kQueue >= kPush, "the queue must hold a block's records");
    static_assert(!(EV64 && (TE || R64)), "FP64 events take their own record queue and carry their times");
    // SlotsLpf keeps ONE escaped dt per lane (esc_dt) and want_step drains it before the next block,
    // which is safe only while a block completes at most one record per lane
    static_assert(!R64 || kPush == 1, "SlotsLpf's single escaped-dt register needs one record per lane per block");
    static_assert(!JOIN || (RESUME && EV64), "lanes join a resumable session of FP64 events (absolute times)");
    static_assert(!NOISE || (RESUME && (EV64 || R64)), "per-filter noise: the resumable and the joining kernels");
    static_assert(!REC || (TRAJ && RESUME), "records are exported beside the poses of a resumable or joining launch");
    const int64_t b = (int64_t)blockIdx.x * kRunBlock + threadIdx.x;
    if (b >= batch) return;
    double qs, rs;
    lane_noise(q_arg, r_arg, b, qs, rs);

    Phase3T<std::conditional_t<EV64, V3, F3>> fe;
    fe.start(init + 6 * b, t_init[b], alpha);
    // a filter that never finished phase 2 (non-finite init: pekf_frontend_init_dev's "not ready")
    // applies no record: its state is left as it was and counts[b] = 0
    const bool ready = init_is_finite(init + 6 * b);
    double rf[6];
    fe.refs(rf);
#pragma unroll
    for (int k = 0; k < 6; ++k) refs[6 * b + k] = rf[k];

    // the filter in its reference frame's basis, covariance as N (pekf_step.hpp), as k_run does it
    Frame Wf;
    make_frame<true>(rf, rf + 3, Wf);
    double x[4];
    Sym4T<double> P;
    if constexpr (JOIN) resume = LiveState<EV64>::joined(state, batch, b);  // the lane's own word, not the launch's
    if constexpr (RESUME) {
        // resumed: the state holds the filter (what enter_ref_basis rotates below is then replaced)
        if (resume) {
            x[0] = 1.0; x[1] = x[2] = x[3] = 0.0;
            P = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0};
        } else {
            load_state<false>(Xio, Pio, b, batch, x, P);
        }
    } else {
        load_state<false>(Xio, Pio, b, batch, x, P);
    }
    // (TRAJ: q_W held for the rows, as k_run's TRAJ kernels hold it; converting late needs it only at the end)
    constexpr bool kLate = TRAJ && PEKF_LIVE_TRAJ_LATE;
    const auto Wr = enter_ref_basis<TRAJ && !kLate>(Wf, refs + 6 * b, false, x, P, rs);
    const StepK kc = step_consts<false, kLoopForm>(qs, rs);
    int32_t applied0 = 0;  // RESUME: the records applied in the session's earlier launches
    if constexpr (RESUME) {
        if (resume) LiveState<EV64>::load(state, batch, b, fe, x, P, applied0);
    }
    const bool fresh = applied0 == 0;

    using Queue = std::conditional_t<EV64, RecordQueue<SlotsF64, kQueue>,
                                     std::conditional_t<R64, RecordQueue<SlotsLpf, kQueue>, RecordQueue<SlotsF32, kQueue>>>;
    __shared__ __attribute__((aligned(16))) unsigned char q_lds[Queue::kBytes];
    Queue queue;
    queue.bind(q_lds);
    int32_t applied = 0;
    bool seen = false;  // JOIN: the lane's column held a message in this launch
    // One filter step for every lane with a queued record: its oldest, Prediction + Correction with
    // the multi-record kernel's arithmetic (the first record of the launch from the loaded |X|^2,
    // every later one lazy; front-end records always carry a magnetometer sample).
    auto filter_step = [&]() {
        const bool has = queue.n > 0;
        double dt;
        const typename Queue::Slot cur = queue.pop(dt);
        auto reload = [&](double *a, double *m) { queue.reload(a, m); };  // rare: the degenerate-Wahba fallback
        OmodMode mode;
        mode.enter();
        if (has) {
            double gy[3], acc[3], mag[3];
            Queue::unpack(cur, gy, acc, mag);
            bool first = applied == 0;
            if constexpr (RESUME) first = first && fresh;
            if constexpr (REC) {
                if (applied < traj_rows) {
                    const int64_t row = (int64_t)applied * batch + b;
                    double2 *g = reinterpret_cast<double2 *>(rec.gd) + 2 * row;
                    double2 *a = reinterpret_cast<double2 *>(rec.am) + 2 * row;
                    g[0] = make_double2(gy[0], gy[1]);
                    g[1] = make_double2(gy[2], dt);
                    a[0] = make_double2(acc[0], acc[1]);
                    a[1] = make_double2(acc[2], mag[0]);
                    rec.my[row] = make_double2(mag[1], mag[2]);
                }
            }
            if (first)
                ekf_record_step<kLoopForm>(x, state_norm2(x), P, Wr, kc, gy, dt, false, acc, mag, reload);
            else  // LAZY
                ekf_record_step<kLoopForm, true>(x, 1.0, P, Wr, kc, gy, dt, false, acc, mag, reload);
            if constexpr (TRAJ) {
                if (applied < traj_rows) {
                    const int64_t row = (int64_t)applied * batch + b;
                    double xo[4] = {x[0], x[1], x[2], x[3]}, qw[4];
                    if constexpr (!kLate) ref_to_world(Wr, x, xo, qw);
                    double2 *o = reinterpret_cast<double2 *>(traj) + 2 * row;
                    o[0] = make_double2(xo[0], xo[1]);
                    o[1] = make_double2(xo[2], xo[3]);
                    if (traj_dt) traj_dt[row] = dt;
                }
            }
            ++applied;
        }
        mode.leave();
    };
    // the pending record (captured by Phase3::event), finished in the queue's form, into the queue
    auto push_pending = [&](const auto &q) {
        bool esc;
        const auto rc = fe.template finish<typename Queue::In>(q, esc);
        if (ready) queue.push(rc, esc, q.dt);
    };
    auto flush = [&]() {
        if (fe.pend) {
            fe.pend = false;
            push_pending(fe.p);
        }
    };

    // wave-uniform: a step while some lane could overflow in the next block, then one more if a quorum
    // of lanes has a record; after the last event until every queue is empty; (R64) while some lane
    // still has an escaped record queued, so the next block cannot queue a second one on that lane
    auto want_step = [&](bool last) {
        const uint64_t queued = __ballot(queue.n > 0);
        return queued != 0 && (last || __any(queue.n > kQueue - kPush) || __popcll(queued) >= kQuorum ||
                               (R64 && !EV64 && __any(queue.esc_queued())));
    };
    auto steps = [&](bool last) {
        // tested before the loop, so a block that runs no step does not pass the loop's header
        if (want_step(last)) {
            do {
                filter_step();
            } while (want_step(last));
        }
    };
    // The events come through the load-ahead ring (pekf_phase3.hpp: event_ring; its null events move no
    // state, with or without TE); nothing is pending after a whole block, and a filter step may follow it.
    event_ring<kRing, PEKF_LIVE_NTL>(
        ev, batch, (uint32_t)b, (int32_t)n_events,
        [&](int k, const EvT &v4) {
            if constexpr (EV64)
                fe.event64(v4);
            else
                fe.template event<TE>(v4);
            if constexpr (JOIN) seen = seen || is_message(v4);
            if ((k + 1) % kFlush == 0) flush();
        },
        steps);
    if constexpr (JOIN) {
        // joined before, or joining now; a lane that has not joined leaves its (zero) state as it is
        if (resume || (ready && seen))
            LiveState<EV64>::store(state, batch, b, fe, x, P, applied0 + applied, LiveState<EV64>::kJoined);
    } else if constexpr (RESUME) {
        LiveState<EV64>::store(state, batch, b, fe, x, P, applied0 + applied);
    }
    counts[b] = applied;
    if (applied == 0) return;  // no record: the state is left as it was (as pekf_run_dev with counts)
    if constexpr (kLate) {
        // the lane's own rows, raw in the reference basis, become ref_to_world's in place (q_W made once)
        RefW Wh;
        Wh.aW = Wr.aW; Wh.b1W = Wr.b1W; Wh.b2W = Wr.b2W;
        Wr.quat(Wh.q);
        const int32_t n_rows = applied < traj_rows ? applied : traj_rows;
        for (int32_t r = 0; r < n_rows; ++r) {
            double2 *o = reinterpret_cast<double2 *>(traj) + 2 * ((int64_t)r * batch + b);
            const double2 lo = o[0], hi = o[1];
            const double xr[4] = {lo.x, lo.y, hi.x, hi.y};
            double xo[4], qw[4];
            ref_to_world(Wh, xr, xo, qw);
            o[0] = make_double2(xo[0], xo[1]);
            o[1] = make_double2(xo[2], xo[3]);
        }
        from_ref_basis(Wh, x, P, lane_r_again(q_arg, b, rs));
    } else {
        from_ref_basis(Wr, x, P, lane_r_again(q_arg, b, rs));
    }
    store_state<false>(Xio, Pio, b, batch, x, P);
}

// What every pekf_live_* entry is handed (include/pekf.h: pekf_live_traj_dev's arguments), filled once by the
// entry and passed to the checks and the launcher below.
struct LiveCall {
    int64_t batch, n_events;
    const void *ev_planes;
    const double *init;
    const int64_t *t_init;
    double alpha;
    double *X, *P;
    double q, r;
    int32_t *counts;
    double *refs;
    uint32_t flags;
    double *traj, *traj_dt;  // read only when traj_rows > 0
    int64_t traj_rows;
    hipStream_t stream;
    const double *noise = nullptr;  // the pekf_live_*_noise_dev entries: the {q, r} plane, in place of q and r
    bool per_filter = false;        // ... and that the call is one of them
    // the pekf_live_*_rec_dev entries: the record planes (RecPlanesArg), traj_rows rows each
    void *rec_gd = nullptr, *rec_am = nullptr, *rec_my = nullptr;
};

// The argument checks every pekf_live_* entry shares, in two halves: sizes, flags and the trajectory arguments
// (before the batch == 0 return), then the launch's limits and pointers (after it).
static inline int check_live_flags(const LiveCall &c) {
    PEKF_CHECK_ARG(c.batch >= 0 && c.n_events >= 0, "negative size");
    PEKF_CHECK_ARG((c.flags & ~(PEKF_EV_TIME_EVENTS | PEKF_EV_F32_RECORDS | PEKF_EV_F64_EVENTS)) == 0, "unknown flags");
    const bool ev64 = (c.flags & PEKF_EV_F64_EVENTS) != 0;
    PEKF_CHECK_ARG(!ev64 || (c.flags & (PEKF_EV_TIME_EVENTS | PEKF_EV_F32_RECORDS)) == 0,
                   "PEKF_EV_F64_EVENTS takes no other flag (FP64 events carry their times; their records are FP64)");
    PEKF_CHECK_ARG(c.traj_rows >= 0 && c.traj_rows < ((int64_t)1 << 31), "traj_rows must be >= 0 and < 2^31");
    PEKF_CHECK_ARG(c.traj_rows == 0 || (c.traj && (uintptr_t)c.traj % 16 == 0),
                   "traj must be a 16-byte aligned pointer when traj_rows > 0");
    PEKF_CHECK_ARG(c.traj_rows == 0 || (uintptr_t)c.traj_dt % 8 == 0, "misaligned traj_dt");
    return PEKF_OK;
}
static inline int check_live_launch(const LiveCall &c) {
    PEKF_CHECK_ARG(c.batch < ((int64_t)1 << 28), "batch must be < 2^28 filters per launch");
    PEKF_CHECK_ARG(c.n_events < ((int64_t)1 << 30), "n_events must be < 2^30 per launch");
    PEKF_CHECK_ARG(c.ev_planes && c.init && c.t_init && c.X && c.P && c.counts && c.refs, "null pointer");
    PEKF_CHECK_ARG((uintptr_t)c.ev_planes % 16 == 0, "misaligned event planes");
    if (c.per_filter)
        PEKF_CHECK_ARG(c.noise && (uintptr_t)c.noise % 16 == 0,
                       "noise must be a 16-byte aligned device pointer to batch {q, r} pairs");
    else
        PEKF_CHECK_ARG(c.r > 0.0, "r must be > 0 (S = P- + rI must be SPD)");
    return PEKF_OK;
}

// The one launch of k_live<TE, R64, EV64, TRAJ, RESUME, JOIN>, by the call's flags (checked by the entry).  Each
// instantiation names the kernels its file holds, and no others (tests/test_omod_listing.py counts them):
//   <TRAJ>              the five of pekf_live_ext_dev's flags, TE x R64 and the FP64-event form (pekf_live.hip
//                       without TRAJ, pekf_live_traj.hip with it);
//   <TRAJ, true>        a resumable launch takes FP64 records, so TE and the FP64-event form (pekf_live_resume.hip);
//   <TRAJ, true, true>  filters join a session of FP64 events only (pekf_live_join.hip).
// Without TRAJ the kernels read none of the trajectory arguments and are handed none.
// NOISE: the same kernels' per-filter-noise forms (pekf_live_resume_noise.hip, pekf_live_join_noise.hip), handed
// c.noise where the others are handed c.q and c.r.
// REC: the TRAJ kernels of a resumable or joining launch that export their records too (pekf_live_rec.hip,
// pekf_live_rec_noise.hip), handed c.rec_gd / c.rec_am / c.rec_my.
template <bool TRAJ, bool RESUME = false, bool JOIN = false, bool NOISE = false, bool REC = false>
int launch_k_live(const LiveCall &c, void *state = nullptr, int32_t resume = 0) {
    static_assert(!NOISE || RESUME, "per-filter noise: the resumable and the joining kernels");
    static_assert(!REC || (TRAJ && RESUME), "records are exported beside the poses of a resumable or joining launch");
    RecPlanes<REC> rec;
    if constexpr (REC)
        rec = {static_cast<double4 *>(c.rec_gd), static_cast<double4 *>(c.rec_am), static_cast<double2 *>(c.rec_my)};
    const dim3 grid(grid_for(c.batch, kRunBlock)), block(kRunBlock);
    NoiseQ<NOISE> q_arg;
    NoiseR<NOISE> r_arg;
    if constexpr (NOISE) {
        q_arg = reinterpret_cast<const double2 *>(c.noise);
    } else {
        q_arg = c.q;
        r_arg = c.r;
    }
    auto launch = [&](auto kernel, const auto *ev) {
        hipLaunchKernelGGL(kernel, grid, block, 0, c.stream, c.batch, c.n_events, ev, c.init, c.t_init, c.alpha, q_arg,
                           r_arg, c.X, c.P, c.counts, c.refs, TRAJ ? c.traj : nullptr, TRAJ ? c.traj_dt : nullptr,
                           TRAJ ? (int32_t)c.traj_rows : 0, state, resume, rec);
    };
    if (JOIN || (c.flags & PEKF_EV_F64_EVENTS))  // the one FP64-event variant
        launch(k_live<false, false, true, TRAJ, RESUME, JOIN, NOISE, REC>, static_cast<const double4 *>(c.ev_planes));
    else if constexpr (RESUME && !JOIN)
        dispatch_bools(
            [&](auto te) {
                launch(k_live<te.value, true, false, TRAJ, true, false, NOISE, REC>, static_cast<const float4 *>(c.ev_planes));
            },
            (c.flags & PEKF_EV_TIME_EVENTS) != 0);
    else if constexpr (!RESUME)
        dispatch_bools(
            [&](auto te, auto r64) {
                launch(k_live<te.value, r64.value, false, TRAJ>, static_cast<const float4 *>(c.ev_planes));
            },
            (c.flags & PEKF_EV_TIME_EVENTS) != 0, (c.flags & PEKF_EV_F32_RECORDS) == 0);
    return launched(JOIN ? "k_live (joining)" : RESUME ? "k_live (resumable)" : "k_live");
}

// launch_k_live<true> (pekf_live_traj.hip)
int launch_live_traj(const LiveCall &c);

// launch_k_live<true, true, join, true, true> (pekf_live_rec_noise.hip), for pekf_live_rec.hip's entries
int launch_live_rec_noise(const LiveCall &c, void *state, int32_t resume, bool join);

}  // namespace pekf
