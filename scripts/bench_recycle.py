#!/usr/bin/env python3
"""Column recycling beside its yardsticks (one JSON object on stdout), HIP events on one stream after a warm-up,
all in this process: a calibrating engine.PhoneSession of 1,048,576 phones (n_cal = 100, FP64 events), started by
one 16-row chunk of every plane, then

  session_chunk   the launches the session makes for a later 16-row chunk of every plane (phase 1 resumed, the
                  correction of both planes, phase 2 resumed, the join), as scripts/bench_magcal.py --chunked times
                  them: what the box pays per chunk anyway
  recycle_<n>     pekf_session_recycle_dev with all three groups on n listed columns: 1, 1,024 (scattered), every
                  column in order and every column scrambled -- 904 B written and 4 B read per listed column
  layout_<n>      pekf_state_layout_dev (k_state_layout, AoS -> SoA: 272 B per filter, pure data movement in
                  coalesced wave tiles) over as many filters as move the same number of bytes: the yardstick the
                  other session kernels are compared with

A recycle is idempotent, so repeating it times the same work.  PEKF_MAGCAL_BENCH_TILE (default 64) scales the batch
down for a quick run.  Nothing is asserted about the times.
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

from bench_aux import HBM, log, timed  # noqa: E402
from bench_magcal import tiled_planes  # noqa: E402

RECYCLE_BYTES = 336 + 160 + 48 + 112 + 8 + 48 + 8 + 4 + 32 + 96 + 48 + 4 + 4   # per listed column, cols[i] included
LAYOUT_BYTES = 160 + 112                                                         # per filter, AoS read + SoA written


def main():
    st = engine.Stream()
    s = st.handle
    K0, rows, n_cal, tile = 16384, 16, 100, int(os.environ.get("PEKF_MAGCAL_BENCH_TILE", "64"))
    K = K0 * tile
    ev = synth.generate_events(np.arange(K0), 3 * rows, seed=12)
    evb = tiled_planes(synth.pack_events64(ev, ev["values"].astype(np.float64)), tile, s)
    row = 32 * K
    ev1, ev2, ev3 = evb.ptr, evb.ptr + row * rows, evb.ptr + row * 2 * rows
    sess = engine.PhoneSession(engine.BatchedEKF(K), n_avg=20, n_cal=n_cal)
    sess.feed_planes(evb, rows, evb, rows, offset2=row * rows, offset3=row * 2 * rows, planes1=evb, n1=rows)
    f = sess.filters
    res = {"phones": K, "n_cal": n_cal, "rows_per_plane": rows, "recycle_bytes_per_column": RECYCLE_BYTES,
           "state_bytes_per_phone": (sess._p1state.nbytes + sess._p2state.nbytes + sess._state.nbytes) // K}

    def chunk():
        check(lib.pekf_magcal_resume_dev(K, rows, ev1, n_cal, sess._cal.ptr, sess._fit.ptr, sess._status.ptr,
                                         EV_F64_EVENTS, sess._p1state.ptr, 1, s))
        for p in (ev2, ev3):
            check(lib.pekf_magcal_apply_dev(K, rows, p, sess._cal.ptr, sess._status.ptr, EV_F64_EVENTS, s))
        check(lib.pekf_frontend_init_resume_dev(K, rows, ev2, sess._t_start.ptr, sess.n_avg, sess._init.ptr,
                                                sess._t_init.ptr, sess._ready.ptr, EV_F64_EVENTS, sess._p2state.ptr, 1, s))
        check(lib.pekf_live_join_dev(K, rows, ev3, sess._init.ptr, sess._t_init.ptr, sess.alpha, f.X.ptr, f.P.ptr, f.q,
                                     f.r, sess._cnt.ptr, sess._refs.ptr, EV_F64_EVENTS, sess._state.ptr, None, None, 0,
                                     None, s))

    a1 = timed(chunk, s, reps=9)
    rng = np.random.default_rng(3)
    lists = {"1": np.array([K // 3], np.int32), "1024": rng.choice(K, min(1024, K), replace=False).astype(np.int32),
             "all_in_order": np.arange(K, dtype=np.int32), "all_scrambled": rng.permutation(K).astype(np.int32)}
    n_max = max(len(c) for c in lists.values()) * RECYCLE_BYTES // LAYOUT_BYTES + 1
    Xa, Pa, Xs, Ps = (engine.DeviceBuffer(b * n_max) for b in (32, 128, 32, 80))
    check(lib.pekf_reset_state_dev(n_max, Xa.ptr, Pa.ptr, s))
    for name, cols in lists.items():
        n = len(cols)
        dev = engine.DeviceBuffer(cols.nbytes).upload(cols)

        def recycle(dev=dev, n=n):
            check(lib.pekf_session_recycle_dev(K, n, dev.ptr, EV_F64_EVENTS, sess._state.ptr, f.X.ptr, f.P.ptr,
                                               sess._refs.ptr, None, None, None, None, sess._p2state.ptr,
                                               sess._t_start.ptr, sess._init.ptr, sess._t_init.ptr, sess._ready.ptr, None,
                                               sess._p1state.ptr, n_cal, sess._cal.ptr, sess._fit.ptr, sess._status.ptr, s))

        n_lay = n * RECYCLE_BYTES // LAYOUT_BYTES + 1

        def layout(n_lay=n_lay):
            check(lib.pekf_state_layout_dev(n_lay, Xa.ptr, Pa.ptr, Xs.ptr, Ps.ptr, 1, s))

        r1, l1, l2, r2 = (timed(recycle, s, reps=9), timed(layout, s, reps=9), timed(layout, s, reps=9),
                          timed(recycle, s, reps=9))
        byts = n * RECYCLE_BYTES
        res["recycle_" + name] = {"columns": n, "recycle_ms": [r1, r2], "layout_filters": n_lay, "layout_ms": [l1, l2],
                                  "bytes": byts, "bytes_predict_ms": byts / (HBM * 1e9) * 1e3}
        log("recycle of %s columns (%d): %.4f / %.4f ms; k_state_layout over the same bytes (%d filters): %.4f / %.4f "
            "ms; the bytes predict %.4f ms" % (name, n, r1, r2, n_lay, l1, l2, res["recycle_" + name]["bytes_predict_ms"]))
    # every column was recycled: the session reads as a new one
    status = sess._status.download((K,), np.int32)
    res["all_fresh"] = bool((status == 1).all() and not sess._ready.download((K,), np.int32).any())
    a2 = timed(chunk, s, reps=9)
    res["session_chunk"] = {"calibrating_ms": [a1, a2]}
    log("the session's launches for a 16-row chunk of every plane: %.3f ms before, %.3f ms after the recycles (every "
        "column fresh again)" % (a1, a2))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
