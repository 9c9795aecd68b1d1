#!/usr/bin/env python3
"""Final (X, P) of a few fused launches -- 40 B records, FP64 records, the fused front-end + filter --
saved to an .npz and printed as SHA-256 prefixes, to compare two builds of libpekf.so bit for bit
(select the build with PEKF_LIB=...).

usage: python scripts/state_digest.py <out.npz>
"""
import hashlib
import os
import sys
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from poseestimationkf_amd import engine, synth

out = {}
for name, batch, steps, missing, prec, layout in [
        ("f64", 65536, 3000, False, "f64", "aos"),
        ("f64_missing", 65536, 3000, True, "f64", "aos"),
        ("mixed_missing", 65536, 3000, True, "mixed", "aos"),
        ("soa_one", 65536, 1, True, "f64", "soa")]:
    win = engine.IMUWindow(batch, 1024).synthesize(seed=7, missing=missing)
    f = engine.BatchedEKF(batch, precision=prec, layout=layout)
    if steps == 1:
        for s in range(8):
            f.run(win, n_steps=1, step0=s)
    else:
        f.run(win, n_steps=steps)
    X, P = f.get_state()
    out[name + "_X"], out[name + "_P"] = X, P
    print(name, float(np.abs(X).sum()), flush=True)

# the FP64-record launch (pekf_run_rec64_dev): plain, and with trajectory output and ragged counts
rec = synth.generate(np.arange(1024), 64, seed=7)
tile = lambda v: np.tile(v.astype(np.float64), (1, 64) + (1,) * (v.ndim - 2))
win = engine.RecordWindow64.from_arrays(tile(rec.gyro), tile(rec.dt_ns), tile(rec.acc), tile(rec.mag),
                                        np.tile(rec.acc0, (64, 1)), np.tile(rec.mag0, (64, 1)))
for name, kw in [("rec64", {}), ("rec64_traj_counts", dict(
        want_traj=True, counts=np.random.default_rng(2).integers(0, 151, size=65536).astype(np.int32)))]:
    f = engine.BatchedEKF(65536)
    tr = f.run(win, n_steps=150, step0=5, **kw)
    out[name + "_X"], out[name + "_P"] = f.get_state()
    if tr is not None:
        out[name + "_traj_last"] = tr[-1]
    print(name, float(np.abs(out[name + "_X"]).sum()), flush=True)

# the fused front-end + filter launch (pekf_live_dev: f32 events, FP64 records)
ev = synth.generate_events(np.arange(8192), 512, seed=11)
f = engine.BatchedEKF(8192)
out["live_counts"], out["live_refs"] = f.run_events(ev)
out["live_X"], out["live_P"] = f.get_state()
print("live", float(np.abs(out["live_X"]).sum()), flush=True)
np.savez(sys.argv[1], **out)
for k in sorted(out):
    print(k, hashlib.sha256(np.ascontiguousarray(out[k]).tobytes()).hexdigest()[:16])
