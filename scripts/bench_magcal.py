#!/usr/bin/env python3
"""Phase 1's two kernels beside their yardstick (one JSON object on stdout), HIP events on one stream after a
warm-up, all in this process:

  magcal        pekf_magcal_dev, 1,048,576 phones x 128 FP64 events: two passes over each phone's first 101 /
                100 messages (32 B each), 148 B written per phone
  frontend_init pekf_frontend_init_ext_dev with stats on the same plane (n_avg = 20, so that 128 mixed events
                make a filter ready and the variance pass runs): the same two-pass shape
  magcal_apply  pekf_magcal_apply_dev, 1,048,576 phones x 1,024 FP64 events: every event read (32 B), 24 B
                written per magnetometer event, 96 B of cal per phone and row chunk (status NULL: every
                phone corrected, whatever the fit of these mixed streams gave)

The planes are 16,384 generated streams tiled x64 on the device (row by row, device-to-device).
PEKF_MAGCAL_BENCH_TILE (default 64) scales the batch down for a quick run.

--chunked: chunked phase 1 instead (pekf_magcal_resume_dev), same box and same process as its yardstick, A B B A
(A: pekf_magcal_dev in one launch; B: the same 128 rows fed in 1, 8 and 64 chunks), each leg the median of three
sessions; then a 16-row chunk fed after every phone has fired, and the launches engine.PhoneSession makes for a
16-row chunk of every plane, with and without n_cal (A B B A).  Beside each time, what the bytes predict at HBM's 8 TB/s: the event rows read once (up to the
8-row block that holds message 101), 24 B per sample written and read back, the 32 B header read and written per
launch, 148 B of outputs per phone in the first launch and per firing phone.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from poseestimationkf_amd import engine, synth  # noqa: E402
from poseestimationkf_amd._lib import EV_F64_EVENTS, check, lib  # noqa: E402

from bench_aux import HBM, bench_events, log, timed  # noqa: E402


def tiled_planes(planes, tile, stream):
    """Host FP64 planes (E, K0, 4) -> a device buffer [E][K0 * tile] double4, each row tiled."""
    E, K0 = planes.shape[:2]
    src = engine.DeviceBuffer(planes.nbytes).upload(planes)
    dst = engine.DeviceBuffer(planes.nbytes * tile)
    row = 32 * K0
    for e in range(E):
        for t in range(tile):
            check(lib.pekf_memcpy_d2d(dst.ptr + row * (e * tile + t), src.ptr + row * e, row, stream))
    check(lib.pekf_stream_sync(stream))
    return dst


def chunked_bytes(K, E, n_cal, chunks):
    """What a session of `chunks` equal chunks over E rows moves, every phone firing at row n_cal (a message per
    row): dict(events, samples, header, outputs, total) bytes"""
    rows_per, rows_read, launches_with_header_read = E // chunks, 0, 0
    for c in range(chunks):
        a = c * rows_per
        if c:
            launches_with_header_read += 1
        if a > n_cal:            # every phone fired in an earlier launch: the header is read, nothing else
            continue
        rows_read += min(rows_per, (n_cal + 1 - a + 7) // 8 * 8)
    launches_storing = sum(1 for c in range(chunks) if c * rows_per <= n_cal)
    b = dict(events=32 * K * rows_read, samples=2 * 24 * n_cal * K,
             header=32 * K * (launches_with_header_read + launches_storing), outputs=2 * 148 * K)
    b["total"] = sum(b.values())
    return b


def chunked(tile):
    """--chunked (module docstring)"""
    st = engine.Stream()
    s = st.handle
    K0, E, n_cal = 16384, 128, 100
    K = K0 * tile
    ev = synth.generate_events(np.arange(K0), E, seed=12)
    evb = tiled_planes(synth.pack_events64(ev, ev["values"].astype(np.float64)), tile, s)
    cal, fit, stb = (engine.DeviceBuffer(n * K) for n in (96, 48, 4))
    cal2, fit2, stb2 = (engine.DeviceBuffer(n * K) for n in (96, 48, 4))
    state = engine.DeviceBuffer(int(lib.pekf_magcal_state_bytes(K, n_cal, EV_F64_EVENTS)))
    row = 32 * K

    def one():
        check(lib.pekf_magcal_dev(K, E, evb.ptr, n_cal, cal.ptr, fit.ptr, stb.ptr, EV_F64_EVENTS, s))

    def session(chunks):
        n = E // chunks
        for c in range(chunks):
            check(lib.pekf_magcal_resume_dev(K, n, evb.ptr + row * n * c, n_cal, cal2.ptr, fit2.ptr, stb2.ptr,
                                             EV_F64_EVENTS, state.ptr, int(c > 0), s))

    res = {"phones": K, "events_per_phone": E, "n_cal": n_cal, "state_bytes_per_phone": state.nbytes // K}
    for chunks in (1, 8, 64):
        a1, b1, b2, a2 = (timed(one, s), timed(lambda: session(chunks), s), timed(lambda: session(chunks), s),
                          timed(one, s))
        same = all(np.array_equal(x.download((x.nbytes,), np.uint8), y.download((y.nbytes,), np.uint8))
                   for x, y in ((cal, cal2), (fit, fit2), (stb, stb2)))
        byts = chunked_bytes(K, E, n_cal, chunks)
        res["chunks_%d" % chunks] = {"one_shot_ms": [a1, a2], "chunked_ms": [b1, b2], "bit_identical": same,
                                     "bytes": byts, "bytes_predict_ms": byts["total"] / (HBM * 1e9) * 1e3}
        log("%2d chunks: one-shot %.3f / %.3f ms, chunked %.3f / %.3f ms (the bytes predict %.3f ms), identical: %s"
            % (chunks, a1, a2, b1, b2, res["chunks_%d" % chunks]["bytes_predict_ms"], same))
    byts1 = K * (32 * (101 + 100) + 148)
    res["one_shot_bytes"] = byts1
    res["one_shot_bytes_predict_ms"] = byts1 / (HBM * 1e9) * 1e3
    res["calibrated"] = int((stb2.download((K,), np.int32) == 0).sum())
    ms = timed(lambda: check(lib.pekf_magcal_resume_dev(K, 16, evb.ptr, n_cal, cal2.ptr, fit2.ptr, stb2.ptr,
                                                        EV_F64_EVENTS, state.ptr, 1, s)), s, reps=9)
    res["chunk_after_all_fired"] = {"rows": 16, "kernel_ms": ms, "bytes": 32 * K,
                                    "bytes_predict_ms": 32 * K / (HBM * 1e9) * 1e3}
    log("a 16-row chunk after every phone has fired: %.4f ms (the header's bytes predict %.4f ms)"
        % (ms, res["chunk_after_all_fired"]["bytes_predict_ms"]))
    del cal, fit, stb, cal2, fit2, stb2, state

    # PhoneSession's launches for a 16-row chunk of every plane, with and without n_cal: the sessions are started by
    # one feed_planes call each, then the launches of a later chunk are enqueued on the timed stream as _launch
    # makes them (phase 1 resumed and the correction of both planes first, with n_cal; then phase 2 and the join)
    rows = 16
    ev1, ev2, ev3 = evb.ptr, evb.ptr + row * 16, evb.ptr + row * 32
    calls = {}
    for name, nc in (("plain", None), ("calibrating", n_cal)):
        sess = engine.PhoneSession(engine.BatchedEKF(K), n_avg=20, n_cal=nc)
        sess.feed_planes(evb, rows, evb, rows, offset2=row * 16, offset3=row * 32,
                         **(dict(planes1=evb, n1=rows) if nc else {}))

        def call(sess=sess, nc=nc):
            f = sess.filters
            if nc:
                check(lib.pekf_magcal_resume_dev(K, rows, ev1, nc, sess._cal.ptr, sess._fit.ptr, sess._status.ptr,
                                                 EV_F64_EVENTS, sess._p1state.ptr, 1, s))
                for p in (ev2, ev3):
                    check(lib.pekf_magcal_apply_dev(K, rows, p, sess._cal.ptr, sess._status.ptr, EV_F64_EVENTS, s))
            check(lib.pekf_frontend_init_resume_dev(K, rows, ev2, sess._t_start.ptr, sess.n_avg, sess._init.ptr,
                                                    sess._t_init.ptr, sess._ready.ptr, EV_F64_EVENTS,
                                                    sess._p2state.ptr, 1, s))
            check(lib.pekf_live_join_dev(K, rows, ev3, sess._init.ptr, sess._t_init.ptr, sess.alpha, f.X.ptr, f.P.ptr,
                                         f.q, f.r, sess._cnt.ptr, sess._refs.ptr, EV_F64_EVENTS, sess._state.ptr,
                                         None, None, 0, None, s))
        calls[name] = call
    a1, b1, b2, a2 = (timed(calls["plain"], s, reps=9), timed(calls["calibrating"], s, reps=9),
                      timed(calls["calibrating"], s, reps=9), timed(calls["plain"], s, reps=9))
    # phase 1: the rows, the header both ways, the samples stored; the correction: the rows, cal and status, and 24 B
    # per corrected magnetometer event at most
    extra = K * (32 * rows + 64 + 24 * rows) + 2 * K * (32 * rows + 96 + 4) + \
        24 * tile * int((ev["types"][16:48] == synth.EV_MAG).sum())
    res["phone_session_chunk"] = {"rows_per_plane": rows, "plain_ms": [a1, a2], "calibrating_ms": [b1, b2],
                                  "extra_bytes_at_most": extra, "extra_bytes_predict_ms": extra / (HBM * 1e9) * 1e3}
    log("PhoneSession's launches, 16 rows of each plane: plain %.3f / %.3f ms, calibrating %.3f / %.3f ms "
        "(phase 1's and the correction's bytes predict at most +%.3f ms)"
        % (a1, a2, b1, b2, res["phone_session_chunk"]["extra_bytes_predict_ms"]))
    print(json.dumps(res))


def main():
    if "--chunked" in sys.argv[1:]:
        return chunked(int(os.environ.get("PEKF_MAGCAL_BENCH_TILE", "64")))
    st = engine.Stream()
    s = st.handle
    K0, tile = 16384, int(os.environ.get("PEKF_MAGCAL_BENCH_TILE", "64"))
    K = K0 * tile
    res = {}

    E = 128
    ev = synth.generate_events(np.arange(K0), E, seed=12)
    host = synth.pack_events64(ev, ev["values"].astype(np.float64))
    evb = tiled_planes(host, tile, s)
    cal, fit, stb = (engine.DeviceBuffer(n * K) for n in (96, 48, 4))
    ms = timed(lambda: check(lib.pekf_magcal_dev(K, E, evb.ptr, 100, cal.ptr, fit.ptr, stb.ptr, EV_F64_EVENTS, s)), s)
    status = stb.download((K,), np.int32)
    byts = K * (32 * (101 + 100) + 148)
    res["magcal"] = {"phones": K, "events_per_phone": E, "kernel_ms": ms, "calibrated": int((status == 0).sum()),
                     "bytes": byts, "gbs": byts / (ms * 1e-3) / 1e9, "hbm_frac": byts / (ms * 1e-3) / 1e9 / HBM}
    log("magcal: %.3f ms, %.0f GB/s" % (ms, res["magcal"]["gbs"]))
    n_avg = 20
    tsb = engine.DeviceBuffer(8 * K).upload(np.tile(ev["t_init"], tile).astype(np.int64))
    ib, tib, sb, rb = (engine.DeviceBuffer(n * K) for n in (48, 8, 96, 4))
    ms = timed(lambda: check(lib.pekf_frontend_init_ext_dev(K, E, evb.ptr, tsb.ptr, n_avg, ib.ptr, tib.ptr, sb.ptr,
                                                            rb.ptr, EV_F64_EVENTS, s)), s)
    last = np.zeros(K0, np.int64)
    for t in (synth.EV_ACC, synth.EV_GYRO, synth.EV_MAG):
        last = np.maximum(last, np.argmax(np.cumsum(ev["types"] == t, axis=0) >= n_avg, axis=0) + 1)
    byts = 32 * (K * E + tile * int(last.sum()))
    res["frontend_init"] = {"filters": K, "events_per_filter": E, "n_avg": n_avg, "kernel_ms": ms,
                            "ready": int(rb.download((K,), np.int32).sum()), "bytes": byts,
                            "gbs": byts / (ms * 1e-3) / 1e9, "hbm_frac": byts / (ms * 1e-3) / 1e9 / HBM}
    log("frontend_init (yardstick): %.3f ms, %.0f GB/s" % (ms, res["frontend_init"]["gbs"]))
    del evb, ib, tib, sb, rb, tsb

    E = 1024
    ev = bench_events(K0, E)
    host = synth.pack_events64(ev, ev["values"].astype(np.float64))
    evb = tiled_planes(host, tile, s)
    del host
    ms = timed(lambda: check(lib.pekf_magcal_apply_dev(K, E, evb.ptr, cal.ptr, None, EV_F64_EVENTS, s)), s)
    n_mag = tile * int((ev["types"] == synth.EV_MAG).sum())   # status NULL: every phone is corrected
    chunks = (E + 63) // 64
    byts = K * E * 32 + n_mag * 24 + K * chunks * 96
    res["magcal_apply"] = {"phones": K, "events_per_phone": E, "kernel_ms": ms, "mag_events_written": n_mag,
                           "bytes": byts, "gbs": byts / (ms * 1e-3) / 1e9, "hbm_frac": byts / (ms * 1e-3) / 1e9 / HBM}
    log("magcal_apply: %.3f ms, %.0f GB/s" % (ms, res["magcal_apply"]["gbs"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
