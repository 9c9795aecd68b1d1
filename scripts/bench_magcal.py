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


def main():
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
