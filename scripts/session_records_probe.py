#!/usr/bin/env python3
"""What the record export of a chunked session costs (pekf_live_resume_rec_dev against the pekf_live_resume_dev
launch with a trajectory that it extends), on the bench_aux.py workload: 16K generated event streams tiled x64 ->
1,048,576 filters x 1,024 events.  Same process, same buffers, A B B A order (A: the TRAJ launch, B: the REC
launch), timed with events on one stream, the 0xFF fill of the output planes inside the timed span and timed
alone as well:

  one chunk            all 1,024 rows in one launch, 342 output rows
  64 chunks of 16      64 resumed launches, 6 output rows each (the planes refilled and reused)
  one-shot             the only other source of the same records: pekf_frontend_ext_dev writing FP64 records, then
                       pekf_run_rec64_dev with counts and a trajectory (FP64 events only)

usage: python3 scripts/session_records_probe.py [--f32] [--filters-log2 N]
(--f32: f32 events instead of FP64 ones, no one-shot; --filters-log2: 2^N filters, default 20.)
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from poseestimationkf_amd import engine, synth, wire  # noqa: E402
from poseestimationkf_amd._lib import EV_F64_EVENTS, EV_TIME_EVENTS, check, lib  # noqa: E402


def main():
    ev64 = "--f32" not in sys.argv
    log2 = int(sys.argv[sys.argv.index("--filters-log2") + 1]) if "--filters-log2" in sys.argv else 20
    K0, E = min(16384, 1 << log2), 1024
    tile = (1 << log2) // K0
    K = K0 * tile
    ev = synth.generate_events(np.arange(K0), E, seed=11)
    packed = synth.pack_events64(ev, wire.server_values(ev["values"])) if ev64 else synth.pack_events(ev)
    flags = EV_F64_EVENTS if ev64 else (EV_TIME_EVENTS if synth.has_time_events(packed) else 0)
    rows_ev = packed.shape[0]
    planes = np.ascontiguousarray(np.tile(packed, (1, tile, 1)))
    row = planes[0].nbytes
    del packed
    evb = engine.DeviceBuffer(planes.nbytes).upload(planes)
    del planes
    init = np.tile(np.concatenate([ev["init_acc"], ev["init_mag"]], axis=1), (tile, 1))
    ib = engine.DeviceBuffer(init.nbytes).upload(init)
    tb = engine.DeviceBuffer(8 * K).upload(np.tile(ev["t_init"], tile).astype(np.int64))
    st = engine.Stream()
    s = st.handle
    R = (rows_ev + 2) // 3
    traj, tdt = engine.DeviceBuffer(32 * R * K), engine.DeviceBuffer(8 * R * K)
    win = engine.RecordWindow64(K, R)
    cnt, refs = engine.DeviceBuffer(4 * K), engine.DeviceBuffer(48 * K)
    state = engine.DeviceBuffer(int(lib.pekf_live_state_bytes(K, flags & EV_F64_EVENTS)))
    f = engine.BatchedEKF(K)
    e0, e1 = engine.Event(), engine.Event()

    def timed(fn):
        e0.record(s)
        fn()
        e1.record(s)
        e1.sync()
        return e0.elapsed_ms(e1)

    def fill(rec, rows):
        for b, w in ((traj, 32), (tdt, 8)) + (((win.gd, 32), (win.am, 32), (win.my, 16)) if rec else ()):
            check(lib.pekf_memset(b.ptr, 0xFF, w * rows * K, s))

    def launch(rec, a, n, rows, resume):
        args = (K, n, evb.ptr + a * row, ib.ptr, tb.ptr, 0.1, f.X.ptr, f.P.ptr, 1.0, 0.1)
        tail = (cnt.ptr, refs.ptr, flags, state.ptr, resume, traj.ptr, tdt.ptr, rows)
        if rec:
            check(lib.pekf_live_resume_rec_dev(*args, None, *tail, win.gd.ptr, win.am.ptr, win.my.ptr, None, s))
        else:
            check(lib.pekf_live_resume_dev(*args, *tail, None, s))

    def session(rec, chunk):
        f.reset(s)
        total = np.zeros(K, np.int64)

        def run():
            for a in range(0, rows_ev, chunk):
                n = min(chunk, rows_ev - a)
                rows = (n + 2) // 3
                fill(rec, rows)
                launch(rec, a, n, rows, int(a > 0))
        ms = timed(run)
        if chunk >= rows_ev:
            total += cnt.download((K,), np.int32)
        return ms, int(total.sum())

    out = {}
    for name, chunk in (("one chunk", rows_ev), ("64 chunks of 16", 16)):
        session(True, chunk), session(False, chunk)                          # warm both
        ms = {False: [], True: []}
        for rec in (False, True, True, False):
            t, n = session(rec, chunk)
            ms[rec].append(t)
            recs = n or out.get("records", 0)
            out["records"] = recs
        fills = {rec: timed(lambda rec=rec: fill(rec, R)) for rec in (False, True)}
        out[name] = dict(traj_ms=ms[False], rec_ms=ms[True], fill_traj_ms=fills[False], fill_rec_ms=fills[True])
    X = f.get_state()[0]
    out["X digest"] = float(np.sum(X * np.arange(1, 5)))
    if ev64:
        err = engine.DeviceBuffer(4).upload(np.zeros(1, np.int32))

        def one_shot():
            check(lib.pekf_frontend_ext_dev(K, rows_ev, evb.ptr, ib.ptr, tb.ptr, 0.1, R, win.gd.ptr, win.am.ptr,
                                            win.my.ptr, None, cnt.ptr, win.refs.ptr, flags, err.ptr, s))
            check(lib.pekf_run_rec64_dev(K, R, R, 0, win.gd.ptr, win.am.ptr, win.my.ptr, win.refs.ptr, f.X.ptr,
                                         f.P.ptr, 1.0, 0.1, traj.ptr, cnt.ptr, s))
        ms = []
        for _ in range(3):
            f.reset(s)
            ms.append(timed(one_shot))
        out["one-shot frontend + run_rec64 with trajectory"] = dict(ms=ms[1:])
        X = f.get_state()[0]
        out["one-shot X digest"] = float(np.sum(X * np.arange(1, 5)))
    print("session_records_probe: %d filters x %d %s event rows, %d output rows" %
          (K, rows_ev, "FP64" if ev64 else "f32", R))
    for key, v in out.items():
        print("  %s: %s" % (key, v))


if __name__ == "__main__":
    main()
