#!/usr/bin/env python3
"""Final (X, P) of a few fused launches -- 40 B records, FP64 records, the fused front-end + filter --
and the outputs of the kernels beside them -- the side outputs over both record types, phases 1 and 2,
the front-end's records -- saved to an .npz and printed as SHA-256 prefixes, to compare two builds of
libpekf.so bit for bit (select the build with PEKF_LIB=...).  The per-call section covers every fixed-width
operator of csrc/pekf_percall.hip on tests/golden/kat.npz's operands -- each row at n = 1 through the resident
service and through a launch per call, the full arrays and a 257-row tiling of them batched -- and
tests/test_percall_service.py's 300 random predict / correct operand sets in both n = 1 modes, a raised case
hashed as its exception text.

usage: python scripts/state_digest.py <out.npz> [percall]      (percall: that section alone)
"""
import hashlib
import os
import sys
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from poseestimationkf_amd import engine, synth

out = {}


def finish():
    np.savez(sys.argv[1], **out)
    for k in sorted(out):
        print(k, hashlib.sha256(np.ascontiguousarray(out[k]).tobytes()).hexdigest()[:16])
    sys.exit(0)


def as_bytes(results):
    """One operator's results -- a tuple of arrays, or ("LinAlgError", text) -- as bytes."""
    return b"".join(r.encode() if isinstance(r, str) else np.ascontiguousarray(r).tobytes() for r in results)


def percall():
    from tests.test_percall_service import _call, _rand_operands
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "kat.npz")) as z:
        kat = {k: z[k] for k in z.files}
    wahba = ("wahba_acc0", "wahba_mag0", "wahba_acc", "wahba_mag", "wahba_ka", "wahba_km")
    ops = [("predict", ("pc_gyro", "pc_dt", "pc_X", "pc_P", "pc_Q", "pc_R")),
           ("correct", ("pc_mag", "pc_acc", "pc_z", "pc_Pm", "pc_K", "pc_acc0", "pc_mag0")),
           ("wahba_quaternion", wahba), ("wahba_rotation", wahba), ("rk4", ("rk4_q0", "rk4_dt", "rk4_w")),
           ("jacobian_a", ("jac_w",)), ("jacobian_b", ("jac_q",)), ("comparator", ("cmp_q1", "cmp_q2")),
           ("rotmat_to_quat", ("r2q_M",))]
    modes = (("service", engine.PERCALL_SERVICE), ("launch", engine.PERCALL_LAUNCH))
    tup = lambda r: r if isinstance(r, tuple) else (r,)
    for name, keys in ops:
        fn, args = getattr(engine, name), [kat[k] for k in keys]
        out["percall_%s_full" % name] = np.frombuffer(as_bytes(tup(fn(*args))), np.uint8)
        tiled = [np.concatenate([a] * -(-257 // len(a)))[:257] for a in args]
        out["percall_%s_257" % name] = np.frombuffer(as_bytes(tup(fn(*tiled))), np.uint8)
        for tag, mode in modes:
            engine.percall_mode(mode)
            rows = [as_bytes(tup(fn(*[a[i] for a in args]))) for i in range(len(args[0]))]
            out["percall_%s_n1_%s" % (name, tag)] = np.frombuffer(b"".join(rows), np.uint8)
        print("per-call", name, flush=True)
    rng = np.random.default_rng(20261017)
    cases = [_rand_operands(rng) for _ in range(300)]
    for tag, mode in modes:
        engine.percall_mode(mode)
        got = [as_bytes(_call(engine.predict, *p)) + as_bytes(_call(engine.correct, *c)) for p, c in cases]
        out["percall_random_%s" % tag] = np.frombuffer(b"".join(got), np.uint8)
    engine.percall_mode(engine.PERCALL_SERVICE)


percall()
if sys.argv[2:] == ["percall"]:
    finish()

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

# the side outputs over 40 B and FP64 records: 150 records from row 5 of a 64-row window (a tail in both
# ring depths, the window replayed)
rec = synth.generate(np.arange(4096), 64, seed=7)
for name, w in [("side", engine.IMUWindow.from_records(rec)),
                ("side64", engine.RecordWindow64.from_arrays(rec.gyro.astype(np.float64), rec.dt_ns,
                                                            rec.acc.astype(np.float64), rec.mag.astype(np.float64),
                                                            rec.acc0, rec.mag0))]:
    out[name + "_gyro_q"], out[name + "_gyro_traj"] = w.gyro_chain(n_steps=150, step0=5, want_traj=True)
    out[name + "_wahba"] = w.wahba_quaternions(n_steps=150, step0=5)
    print(name, float(np.abs(out[name + "_gyro_q"]).sum()), flush=True)
# the same with every seventh record's dt escaped to the side plane (the LONGDT gyro chain)
esc = np.zeros(rec.dtw.shape, bool)
esc.reshape(-1)[::7] = True
rec.dtx = np.where(esc, 3.0e9 + (rec.dtw & synth.DT_MASK), 0.0)
rec.dtw = np.where(esc, rec.dtw | synth.DT_ESCAPE, rec.dtw).astype(np.uint32)
out["side_esc_gyro_q"], out["side_esc_gyro_traj"] = engine.IMUWindow.from_records(rec).gyro_chain(
    n_steps=150, step0=5, want_traj=True)

# phases 2 and 3 of the front-end (pekf_frontend_init_ext_dev with stats, pekf_frontend_ext_dev) and phase 1
# (pekf_magcal_dev), f32 and FP64 events; row counts that leave a partial last block
ev2 = synth.generate_events(np.arange(4096), 523, seed=8)
ev1 = synth.generate_calibration_events(4096, 103, seed=3)
for form in ("f32", "f64"):
    for k, v in engine.frontend_init(ev2, n_avg=100, events=form).items():
        out["init_%s_%s" % (form, k)] = v
    cal = engine.calibrate_magnetometer(ev1, n_cal=100, events=form)
    for k in ("bias", "W", "fit", "status"):
        out["magcal_%s_%s" % (form, k)] = cal[k]
    win, counts = engine.run_frontend(ev, events=form)
    dt = np.float64 if form == "f64" else np.float32
    written = np.arange(win.window)[:, None] < counts[None, :]   # the rows past a filter's count are not written
    for name, buf, width in [("gd", win.gd, 4), ("am", win.am, 4), ("my", win.my, 2)]:
        out["frontend_%s_%s" % (form, name)] = np.where(written[..., None],
                                                        buf.download((win.window, win.batch, width), dt), 0)
    out["frontend_%s_refs" % form] = win.refs.download((win.batch, 6), np.float64)
    out["frontend_%s_counts" % form] = counts
    print("front-end", form, int(counts.sum()), flush=True)
finish()
