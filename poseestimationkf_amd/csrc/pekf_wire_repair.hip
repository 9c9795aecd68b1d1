// pekf_wire_repair.hip -- the phones pekf_wire_events_*_dev stopped, taken over by the host
// (pekf_wire_gather_frames_dev, pekf_wire_patch_dev): the rare path beside pekf_wire_dev.hip, in a file of its own
// so that the parser's object and listings hold the kernels they held.
//
// The device parser refuses a frame that is not in the client's own form and stops that phone alone: its rows
// from the frame on are no-message events, its counts those up to it, bad_frame[b] the frame.  The server does
// the same per phone: it runs one process per client (KFS/Server.cpp:58, :93), reads with std::stod any form
// strtod reads, and where std::stod / std::stoll throw, that client's process ends -- no file of KFS/ has a try
// -- and nobody else's.  So the host reads the stopped phones' frames from bad_frame on
// (pekf_wire_parse_frames, pekf_wire.cpp) and writes what it made of them into those columns:
//   k_wire_gather_frames  the listed columns' frames, [n_frames][batch][100] -> [n_cols][frames][100], so that one
//                         download brings the refused phones' frames and nobody else's;
//   k_wire_patch          the host-built event cells into the listed columns' rows, the no-message event after
//                         them, and the columns' counts, first phase-2 time and bad_frame;
//   k_wire_row_bounds     PEKF_WIRE_FRAME_ROWS' row bounds afresh from the planes (the parse's own are the maximum
//                         over what every wave saw, a stopped phone's later chunks included, and cannot be lowered
//                         from the host without every other phone's rows).
// Pure data movement, nothing here is tuned: a patch moves 96 B per listed column and row.
#include "pekf_internal.hpp"
#include "pekf_phase3.hpp"

namespace pekf {

constexpr int kRepairBlock = 256;
constexpr int kFrameDwords = PEKF_WIRE_FRAME_BYTES / 4;  // 25: a frame is whole dwords, and 4-byte aligned

// One lane per dword of the output: 25 adjacent lanes read one frame, the output is written contiguously.
__global__ __launch_bounds__(kRepairBlock) void k_wire_gather_frames(int64_t batch, int64_t n_out,
                                                                     const uint32_t *__restrict__ frames,
                                                                     int64_t n_cols, const int32_t *__restrict__ cols,
                                                                     int64_t frame0, uint32_t *__restrict__ out) {
    // (n_out: the frames gathered per column, [frame0, frame0 + n_out))
    const int64_t j = (int64_t)blockIdx.x * kRepairBlock + threadIdx.x;
    if (j >= n_cols * n_out * kFrameDwords) return;
    const int64_t fr = j / kFrameDwords, d = j % kFrameDwords;
    const int64_t i = fr / n_out, f = frame0 + fr % n_out;
    const int64_t b = cols[i];
    out[j] = b >= 0 && b < batch ? frames[(f * batch + b) * kFrameDwords + d] : 0u;
}

struct PatchArgs {
    int64_t batch, n_cols, cell_rows;
    const pekf_wire_patch_col *cols;
    const double4 *cells;  // [3][cell_rows][n_cols]
    int64_t e1_max, e2_max, e3_max;
    double4 *ev1, *ev2, *ev3;  // ev1 null: no phase-1 plane
    int64_t *first_t2;
    int32_t *n1, *n2, *n3;
    int32_t *bad_frame;
};

// One lane per listed column (adjacent records: adjacent cells, and for adjacent columns adjacent stores), one
// block row per plane; the first block row writes the column's counts as well.  Every store is to a row in
// [from_row, e_max) of a column in [0, batch).
__global__ __launch_bounds__(kRepairBlock) void k_wire_patch(PatchArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kRepairBlock + threadIdx.x;
    if (i >= a.n_cols) return;
    const pekf_wire_patch_col *c = a.cols + i;
    const int64_t b = c->col;
    if (b < 0 || b >= a.batch) return;  // (the entry refuses these; a lane never stores outside the planes)
    const int p = blockIdx.y;
    if (p == 0) {
        if (a.n1) a.n1[b] = c->n[0];
        a.n2[b] = c->n[1];
        a.n3[b] = c->n[2];
        a.first_t2[b] = c->first_t2;
        if (a.bad_frame) a.bad_frame[b] = c->bad_frame;
    }
    // (selects of values: arrays in the argument, indexed by the plane, would be copied to scratch)
    double4 *ev = p == 0 ? a.ev1 : (p == 1 ? a.ev2 : a.ev3);
    if (!ev) return;  // uniform: a launch argument
    const int64_t e_max = p == 0 ? a.e1_max : (p == 1 ? a.e2_max : a.e3_max);
    const int32_t from = c->from_row[p], given = c->n_cells[p];  // (global loads at a uniform offset)
    const int64_t r0 = from < 0 ? 0 : from;
    const int64_t nc = given < a.cell_rows ? given : a.cell_rows;
    const double4 *cell = a.cells + (int64_t)p * a.cell_rows * a.n_cols + i;
    const double4 none = ev64_null();
    int64_t r = r0;
    for (int64_t j = 0; j < nc && r < e_max; ++j, ++r) ev[r * a.batch + b] = cell[j * a.n_cols];
    for (; r < e_max; ++r) ev[r * a.batch + b] = none;
}

// bounds[0] = 1 + the last row of ev2 holding a message, [1] = n_rows - the first row of ev3 holding one (0:
// none), [2] = [0]'s of ev1 (null: left 0): one block per row, its lanes over the columns.
__global__ __launch_bounds__(kRepairBlock) void k_wire_row_bounds(int64_t batch, int64_t n_rows,
                                                                  const double4 *__restrict__ ev1,
                                                                  const double4 *__restrict__ ev2,
                                                                  const double4 *__restrict__ ev3,
                                                                  int32_t *__restrict__ bounds) {
    const int64_t r = blockIdx.x;
    bool m1 = false, m2 = false, m3 = false;
    for (int64_t b = threadIdx.x; b < batch; b += kRepairBlock) {
        m2 |= !ev64_none(ev2[r * batch + b]);
        m3 |= !ev64_none(ev3[r * batch + b]);
        if (ev1) m1 |= !ev64_none(ev1[r * batch + b]);
    }
    if (__any(m2) && (threadIdx.x & 63) == 0) atomicMax(bounds, (int32_t)r + 1);
    if (__any(m3) && (threadIdx.x & 63) == 0) atomicMax(bounds + 1, (int32_t)(n_rows - r));
    if (__any(m1) && (threadIdx.x & 63) == 0) atomicMax(bounds + 2, (int32_t)r + 1);
}

}  // namespace pekf

using namespace pekf;

extern "C" int pekf_wire_gather_frames_dev(int64_t batch, int64_t n_frames, const void *frames, int64_t n_cols,
                                           const int32_t *cols, int64_t frame0, void *out, void *stream) {
    PEKF_CHECK_ARG(batch >= 0 && n_frames >= 0 && n_cols >= 0, "negative size");
    PEKF_CHECK_ARG(frame0 >= 0 && frame0 <= n_frames, "frame0 must lie in [0, n_frames]");
    PEKF_CHECK_ARG(batch < ((int64_t)1 << 28) && n_frames < ((int64_t)1 << 31), "batch must be < 2^28, n_frames < 2^31");
    PEKF_CHECK_ARG((uintptr_t)frames % 4 == 0 && (uintptr_t)out % 4 == 0, "misaligned buffers");
    const int64_t n_out = n_frames - frame0;
    if (n_cols == 0 || n_out == 0 || batch == 0) return PEKF_OK;
    PEKF_CHECK_ARG(frames && cols && out, "null pointer");
    PEKF_CHECK_ARG(n_cols <= batch, "cols lists distinct columns: n_cols must be <= batch");
    const int64_t blocks = (n_cols * n_out * kFrameDwords + kRepairBlock - 1) / kRepairBlock;
    PEKF_CHECK_ARG(blocks < ((int64_t)1 << 31), "more than 2^31 blocks: gather fewer columns or frames per call");
    hipLaunchKernelGGL(k_wire_gather_frames, dim3((unsigned)blocks), dim3(kRepairBlock), 0, as_stream(stream), batch,
                       n_out, static_cast<const uint32_t *>(frames), n_cols, cols, frame0,
                       static_cast<uint32_t *>(out));
    return launched("k_wire_gather_frames");
}

extern "C" int pekf_wire_patch_dev(int64_t batch, int64_t n_cols, const pekf_wire_patch_col *cols,
                                   const pekf_wire_patch_col *cols_dev, int64_t cell_rows, const void *cells, int64_t e1_max, int64_t e2_max, int64_t e3_max, void *ev1,
                                   void *ev2, void *ev3, int64_t *first_t2, int32_t *n1, int32_t *n2, int32_t *n3,
                                   int32_t *bad_frame, int64_t n_rows, int32_t *row_bounds, void *stream) {
    PEKF_CHECK_ARG(batch >= 0 && n_cols >= 0 && cell_rows >= 0 && e1_max >= 0 && e2_max >= 0 && e3_max >= 0 &&
                       n_rows >= 0,
                   "negative size");
    PEKF_CHECK_ARG(batch < ((int64_t)1 << 28), "batch must be < 2^28 phones per launch");
    PEKF_CHECK_ARG(cell_rows < ((int64_t)1 << 31) && e1_max < ((int64_t)1 << 31) && e2_max < ((int64_t)1 << 31) &&
                       e3_max < ((int64_t)1 << 31),
                   "cell_rows and e_max must be < 2^31");
    PEKF_CHECK_ARG((uintptr_t)ev1 % 16 == 0 && (uintptr_t)ev2 % 16 == 0 && (uintptr_t)ev3 % 16 == 0 &&
                       (uintptr_t)cells % 16 == 0 && (uintptr_t)cols_dev % 8 == 0,
                   "misaligned buffers");
    PEKF_CHECK_ARG((ev1 != nullptr) == (n1 != nullptr), "the phase-1 plane needs ev1 and n1 together");
    PEKF_CHECK_ARG(!row_bounds || (n_rows <= e2_max && n_rows <= e3_max && (!ev1 || n_rows <= e1_max)),
                   "row_bounds: the planes need n_rows rows (n_rows <= e_max)");
    if (batch == 0 || (n_cols == 0 && !row_bounds)) return PEKF_OK;
    PEKF_CHECK_ARG((ev2 || e2_max == 0) && (ev3 || e3_max == 0) && (ev1 || !n1 || e1_max == 0), "null pointer");
    PEKF_CHECK_ARG(n_cols == 0 || (cols && cols_dev && first_t2 && n2 && n3 && (cells || cell_rows == 0)), "null pointer");
    PEKF_CHECK_ARG(n_cols <= batch, "cols lists distinct columns: n_cols must be <= batch");
    for (int64_t i = 0; i < n_cols; ++i) {
        const pekf_wire_patch_col &c = cols[i];
        if (c.col < 0 || c.col >= batch)
            return set_error(PEKF_ERR_INVALID, "record %lld: column %d outside [0, %lld)", (long long)i, c.col,
                             (long long)batch);
        for (int p = 0; p < 3; ++p)
            if (c.from_row[p] < 0 || c.n_cells[p] < 0 || c.n_cells[p] > cell_rows)
                return set_error(PEKF_ERR_INVALID,
                                 "record %lld: negative from_row or n_cells, or n_cells above cell_rows", (long long)i);
    }
    hipStream_t st = as_stream(stream);
    if (n_cols) {
        const PatchArgs a = {batch,
                             n_cols,
                             cell_rows,
                             cols_dev,
                             static_cast<const double4 *>(cells),
                             e1_max,
                             e2_max,
                             e3_max,
                             static_cast<double4 *>(ev1),
                             static_cast<double4 *>(ev2),
                             static_cast<double4 *>(ev3),
                             first_t2,
                             n1,
                             n2,
                             n3,
                             bad_frame};
        hipLaunchKernelGGL(k_wire_patch, dim3(grid_for(n_cols, kRepairBlock), 3), dim3(kRepairBlock), 0, st, a);
        if (int err = launched("k_wire_patch")) return err;
    }
    if (row_bounds) {
        PEKF_HIP(hipMemsetAsync(row_bounds, 0, 3 * sizeof(int32_t), st));
        if (n_rows) {
            hipLaunchKernelGGL(k_wire_row_bounds, dim3((unsigned)n_rows), dim3(kRepairBlock), 0, st, batch, n_rows,
                               static_cast<const double4 *>(ev1), static_cast<const double4 *>(ev2),
                               static_cast<const double4 *>(ev3), row_bounds);
            return launched("k_wire_row_bounds");
        }
    }
    return PEKF_OK;
}
