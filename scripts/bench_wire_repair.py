#!/usr/bin/env python3
"""What refused="repair" costs the wire session: engine.run_wire_session on 65,536 phones x
(700 phase-2 + 1,024 phase-3) frames resident on the device -- wire_probe.py --session's frames -- wall clock in
the calling thread, one JSON line.

usage: python3 scripts/bench_wire_repair.py MODE [reps] [--refuse N] [--tile T] [--frames FILE]

MODE: parent (no refused= argument: for a tree from before it, chosen with PEKF_TREE=<its root>), raise, repair.
--refuse N: N phones (at random) get one frame (at random) with a value in a form only the host reads ("0x1p3");
repair mode only.  The added time is split by timing the engine's steps: the gather + download of the refused
phones' frames, wire.parse_frames, and the rest (the host walk, the cells' upload, the patch launch and its sync).
--frames FILE: the generated 1,024 phones' frames, kept in / read from an .npy file (the text takes a minute to
print; an A B B A over several processes generates it once).  --tile T: phones = 1,024 T (default 64)."""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.environ.get("PEKF_TREE") or os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from poseestimationkf_amd import engine, synth, wire  # noqa: E402
from poseestimationkf_amd._lib import check, lib  # noqa: E402


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def frames_of_1024(path):
    if path and os.path.exists(path):
        return np.load(path)
    K0, E2, E3 = 1024, 700, 1024
    ph2 = synth.generate_events(np.arange(K0), E2, seed=71)
    ph3 = synth.generate_events(np.arange(K0), E3, seed=72)
    ph3 = dict(ph3, times=ph3["times"] - ph3["t_init"][None, :] + ph2["times"][-1][None, :])
    texts = [wire.events_text(ph2["types"][:, k], ph2["values"][:, k], ph2["times"][:, k], phase=2) +
             wire.events_text(ph3["types"][:, k], ph3["values"][:, k], ph3["times"][:, k], phase=3) for k in range(K0)]
    fr = wire.frames(texts)
    if path:
        np.save(path, fr)
    return fr


def main():
    mode = sys.argv[1]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 5
    refuse, tile = _arg("--refuse", 0), _arg("--tile", 64)
    fr0 = frames_of_1024(_arg("--frames", ""))
    fr = np.ascontiguousarray(np.tile(fr0, (1, tile, 1)))
    F, K = fr.shape[:2]
    fb = engine.DeviceBuffer(fr.nbytes).upload(fr)
    if refuse:   # one frame of each chosen phone, its first value in a form the device parser leaves to the host
        rng = np.random.default_rng(9)
        for k, f in zip(rng.choice(K, refuse, replace=False), rng.integers(0, F, refuse)):
            head, rest = fr[f, k].tobytes().decode().rstrip().split(":", 1)
            odd = (head + ":0x1p3," + rest.split(",", 1)[1]).ljust(99) + "\n"
            one = np.frombuffer(odd.encode(), np.uint8)
            check(lib.pekf_memcpy_h2d(fb.ptr + 100 * (int(f) * K + int(k)), one.ctypes.data, 100, None))
    del fr
    split = dict(download=0.0, parse=0.0, repair=0.0)
    if mode == "repair":   # the repair path, timed where the engine calls its steps

        def timed(key, fn):
            def f(*a, **kw):
                t = time.perf_counter()
                out = fn(*a, **kw)
                split[key] += time.perf_counter() - t
                return out
            return f
        engine._refused_frames = timed("download", engine._refused_frames)
        wire.parse_frames = timed("parse", wire.parse_frames)
        engine._repair_wire = timed("repair", engine._repair_wire)
    kw = {} if mode == "parent" else dict(refused=mode)
    f = engine.BatchedEKF(K)
    ms, out = [], None
    for _ in range(reps + 1):
        f.reset()
        check(lib.pekf_device_sync())
        for key in split:
            split[key] = 0.0
        t = time.perf_counter()
        out = engine.run_wire_session((fb, F, K), f, **kw)
        ms.append((time.perf_counter() - t) * 1e3)
    X, _ = f.get_state()
    res = dict(bench="wire session", mode=mode, phones=K, frames_per_phone=F, refused_phones=refuse,
               ms_median=float(np.median(ms[1:])), ms_min=float(min(ms[1:])), ms_max=float(max(ms[1:])), ms=ms,
               ready=int(out["ready"].sum()), records=int(out["counts"].sum()),
               digest=float(np.abs(X[np.isfinite(X).all(axis=1)]).sum()))
    if mode == "repair":
        res.update(repaired=int(out["repaired"].sum()), stopped=int((out["bad_frame"] >= 0).sum()),
                   # the last call's repair: the refused phones' frames fetched (gather launch + download), the host
                   # parse, and the rest -- the walk, the cells' upload, the patch launch, its sync and the bounds
                   last_call_ms=dict(download=split["download"] * 1e3, host_parse=split["parse"] * 1e3,
                                     walk_upload_patch=(split["repair"] - split["download"] - split["parse"]) * 1e3,
                                     repair_total=split["repair"] * 1e3))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
