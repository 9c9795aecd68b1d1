#!/usr/bin/env python3
"""The fused live launch with a pose per record (pekf_live_traj_dev) against the plain fused launch and against
the split route that gave the same trajectory before it, on the same events: 16,384 generated phone streams x
1,024 events tiled x64 = 1,048,576 filters (the shape of scripts/bench_aux.py's front-end lines).

    bench_live_traj.py [name=path/to/libpekf.so ...]

Every library named is loaded into this one process (ctypes; they share the HIP runtime, the event planes and the
output buffers) and timed in the order given, so `base=... new=... new=... base=...` is a same-box A B B A with
nothing but the kernels differing.  Without arguments: the tree's own library, once.  Per library, kernel times by
HIP events on the launch stream (median of 5 after a warm-up launch):

  live_default              pekf_live_dev (f32 events, FP64 records), no trajectory
  live_<form>               pekf_live_ext_dev, form = f64rec / f32rec / ev64
  traj_<form>               pekf_live_traj_dev with traj and traj_dt, traj_rows = the most records of any filter
  split_f32 / split_ev64    pekf_frontend_ext_dev + pekf_run_dev / pekf_run_rec64_dev with trajectory and counts
                            (once, with the first library that has pekf_live_traj_dev, and again after the last)

A library without pekf_live_traj_dev (a build of an earlier commit) runs its live_* lines only.  One JSON object
on stdout; traj_sha1 is of the first three trajectory and dt rows, to compare builds."""
from __future__ import annotations

import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from poseestimationkf_amd import _lib, engine, synth, wire  # noqa: E402
from poseestimationkf_amd._lib import EV_F32_RECORDS, EV_F64_EVENTS, check  # noqa: E402

FORMS = (("f64rec", 0), ("f32rec", EV_F32_RECORDS), ("ev64", EV_F64_EVENTS))


def log(m):
    print("[live_traj] " + m, file=sys.stderr, flush=True)


def load(path):
    lib = ctypes.CDLL(path)
    for name, argtypes in _lib.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.argtypes = argtypes
            fn.restype = ctypes.c_int
    return lib


def timed(fn, stream, reps=5):
    e0, e1 = engine.Event(), engine.Event()
    fn()
    check(_lib.lib.pekf_stream_sync(stream))
    out = []
    for _ in range(reps):
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.sync()
        out.append(e0.elapsed_ms(e1))
    return float(np.median(out))


def tiled(planes, tile):
    """[E][K0][4] host planes -> a device buffer [E][K0 * tile][4] (each row copied tile times on the device)"""
    E, K0 = planes.shape[:2]
    row = planes[0].nbytes
    src = engine.DeviceBuffer(planes.nbytes).upload(planes)
    dst = engine.DeviceBuffer(planes.nbytes * tile)
    for e in range(E):
        for t in range(tile):
            check(_lib.lib.pekf_memcpy_d2d(dst.ptr + (e * tile + t) * row, src.ptr + e * row, row, None))
    check(_lib.lib.pekf_device_sync())
    return dst


def ok(status):
    if status != 0:
        raise RuntimeError("libpekf status %d" % status)


def main(argv):
    libs = [a.split("=", 1) for a in argv] or [["tree", _lib.LIB_PATH]]
    loaded = {path: load(path) for _, path in libs}
    st = engine.Stream()
    s = st.handle
    K0, E, tile = int(os.environ.get("PEKF_TRAJ_K0", 16384)), 1024, int(os.environ.get("PEKF_TRAJ_TILE", 64))
    log("generating %d x %d events" % (K0, E))
    ev = synth.generate_events(np.arange(K0), E, seed=11)
    K = K0 * tile
    init = np.tile(np.concatenate([ev["init_acc"], ev["init_mag"]], axis=1), (tile, 1))
    tinit = np.tile(ev["t_init"], tile).astype(np.int64)
    ib = engine.DeviceBuffer(init.nbytes).upload(init)
    tb = engine.DeviceBuffer(tinit.nbytes).upload(tinit)
    p32 = synth.pack_events(ev)
    assert not synth.has_time_events(p32)
    ev32, ev64 = tiled(p32, tile), tiled(synth.pack_events64(ev, wire.server_values(ev["values"])), tile)
    cnt, refs = engine.DeviceBuffer(4 * K), engine.DeviceBuffer(48 * K)
    f = engine.BatchedEKF(K)
    ok(loaded[libs[0][1]].pekf_live_dev(K, E, ev32.ptr, ib.ptr, tb.ptr, 0.1, f.X.ptr, f.P.ptr, 1.0, 0.1, cnt.ptr,
                                        refs.ptr, None, s))
    check(_lib.lib.pekf_stream_sync(s))
    counts = cnt.download((K,), np.int32)
    n_rec, recs = int(counts.max()), int(counts.sum())
    traj, tdt = engine.DeviceBuffer(32 * n_rec * K), engine.DeviceBuffer(8 * n_rec * K)
    res = {"filters": K, "events_per_filter": E, "records": recs, "traj_rows": n_rec, "runs": []}
    log("%d filters, %d records, %d trajectory rows" % (K, recs, n_rec))

    def split(lib):
        out = {}
        r_max = E // 3 + 1
        err = engine.DeviceBuffer(4).upload(np.zeros(1, np.int32))
        win = engine.IMUWindow(K, r_max)
        fe = timed(lambda: ok(lib.pekf_frontend_ext_dev(K, E, ev32.ptr, ib.ptr, tb.ptr, 0.1, r_max, win.gd.ptr,
                                                        win.am.ptr, win.my.ptr, None, cnt.ptr, win.refs.ptr, 0,
                                                        err.ptr, s)), s)
        run = timed(lambda: ok(lib.pekf_run_dev(K, n_rec, r_max, 0, win.gd.ptr, win.am.ptr, win.my.ptr, win.refs.ptr,
                                                f.X.ptr, f.P.ptr, 1.0, 0.1, traj.ptr, cnt.ptr, 0, s)), s)
        out["split_f32"] = {"frontend_ms": fe, "run_traj_ms": run, "ms": fe + run}
        del win
        w64 = engine.RecordWindow64(K, r_max)
        fe = timed(lambda: ok(lib.pekf_frontend_ext_dev(K, E, ev64.ptr, ib.ptr, tb.ptr, 0.1, r_max, w64.gd.ptr,
                                                        w64.am.ptr, w64.my.ptr, None, cnt.ptr, w64.refs.ptr,
                                                        EV_F64_EVENTS, err.ptr, s)), s)
        run = timed(lambda: ok(lib.pekf_run_rec64_dev(K, n_rec, r_max, 0, w64.gd.ptr, w64.am.ptr, w64.my.ptr,
                                                      w64.refs.ptr, f.X.ptr, f.P.ptr, 1.0, 0.1, traj.ptr, cnt.ptr, s)), s)
        out["split_ev64"] = {"frontend_ms": fe, "run_traj_ms": run, "ms": fe + run}
        assert int(err.download((1,), np.int32)[0]) == 0
        return out

    split_lib = None
    for name, path in libs:
        lib = loaded[path]
        has_traj = hasattr(lib, "pekf_live_traj_dev")
        run = {"lib": name}
        run["live_default"] = timed(lambda: ok(lib.pekf_live_dev(K, E, ev32.ptr, ib.ptr, tb.ptr, 0.1, f.X.ptr, f.P.ptr,
                                                                 1.0, 0.1, cnt.ptr, refs.ptr, None, s)), s)
        # the plain lines first, then the trajectory ones: a TRAJ launch writes gigabytes, and a plain line timed
        # right after one ran 3-4 % slower than the same kernel timed after plain ones (profiles/r12/live_traj/)
        for form, flags in FORMS:
            evb = ev64 if flags & EV_F64_EVENTS else ev32
            run["live_" + form] = timed(lambda: ok(lib.pekf_live_ext_dev(
                K, E, evb.ptr, ib.ptr, tb.ptr, 0.1, f.X.ptr, f.P.ptr, 1.0, 0.1, cnt.ptr, refs.ptr, flags, None, s)), s)
        for form, flags in FORMS if has_traj else ():
            evb = ev64 if flags & EV_F64_EVENTS else ev32
            run["traj_" + form] = timed(lambda: ok(lib.pekf_live_traj_dev(
                K, E, evb.ptr, ib.ptr, tb.ptr, 0.1, f.X.ptr, f.P.ptr, 1.0, 0.1, cnt.ptr, refs.ptr, flags, traj.ptr,
                tdt.ptr, n_rec, None, s)), s)
            h = hashlib.sha1(traj.download((3, K, 4), np.float64).tobytes())
            h.update(tdt.download((3, K), np.float64).tobytes())
            run["traj_sha1_" + form] = h.hexdigest()
        if has_traj and split_lib is None:
            split_lib = lib
            run.update(split(lib))
        log(json.dumps(run))
        res["runs"].append(run)
    if split_lib is not None:
        res["split_again"] = split(split_lib)
        log(json.dumps(res["split_again"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])
