#!/usr/bin/env python3
"""Measurements of the kernels beside the headline fused run (one JSON object on stdout).

  frontend      pekf_frontend_dev: raw phone events -> records; HBM-bound:
                16 B read per event + 40 B written per record
  frontend_then_filter   the filter over those records (pekf_run_dev with counts): the split pipeline
  live          pekf_live_dev: the same events -> filter in one launch (no record window); 16 B read per
                event + the state once (PEKF_AUX_ONLY=live stops after it, =side after wahba_stream)
  live_resume   PEKF_AUX_ONLY=live_resume, that case alone: pekf_live_resume_dev, the same session fed in 1, 8, 64
                and 342 chunks beside the one launch, f32 and FP64 events (profiles/r15/live_resume/)
  phone_session PEKF_AUX_ONLY=phone_session, that case alone: pekf_frontend_init_resume_dev + pekf_live_join_dev per
                chunk beside one-shot phase 2 + pekf_live_resume_dev, 1, 8 and 64 chunks (profiles/r16/live_start/)
  noise_per_filter PEKF_AUX_ONLY=noise_per_filter, that case alone: the per-filter-noise kernels beside the scalar ones,
                same-box A B B A: the multi-record launch at config 3's shape, and a LiveSession's launches over
                1,048,576 x 1,024 f32 events as one chunk and as 64 (profiles/r21/noise_per_filter/)
  session_move  PEKF_AUX_ONLY=session_move, that case alone: pekf_session_export_dev / pekf_session_import_dev on 1,
                1,024 and every column of a 1,048,576-phone PhoneSession beside snapshot + restore, and a chunk's
                launches in a sparse session against the compact one that adopted its phones
                (profiles/r22/session_move/)
  gyro_chain    pekf_gyro_chain_dev (§8f-3): 16 B read per filter-record
  wahba_stream  pekf_wahba_stream_dev (§8f-3): 24 B read + 32 B written per filter-record
  predict_dev / correct_dev   per-call operators at n = 1M items (device pointers)
  online_step_aos / _soa   1M filters x 1 record per launch (state through HBM every launch)
  ctypes_call / dropin_call   host-pointer per-call latency at n = 1 via ctypes / via the CPython
                binding the drop-in modules use (the path main_file.py takes)
  c1_loop       config 1: main_file.py's loop over the committed log, drop-ins vs NumPy on the host

Kernel times are HIP events on the launch stream; run under rocprofv3 --kernel-trace --stats
for the per-kernel summary committed in profiles/.
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from poseestimationkf_amd import engine, synth  # noqa: E402
from poseestimationkf_amd._lib import check, lib  # noqa: E402

HBM = 8000.0


def log(m):
    print("[aux] " + m, file=sys.stderr, flush=True)


def timed(fn, stream, reps=3):
    e0, e1 = engine.Event(), engine.Event()
    fn()
    check(lib.pekf_stream_sync(stream))
    out = []
    for _ in range(reps):
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.sync()
        out.append(e0.elapsed_ms(e1))
    return float(np.median(out))


def bench_events(K0=16384, E=1024):
    """The generated event streams of the front-end measurements (seed 11); PEKF_EV64_CACHE names an .npz that
    keeps them between the runs of an A/B (scripts/bench_ev64.py reads and writes the same file)."""
    cache = os.environ.get("PEKF_EV64_CACHE")
    if cache and os.path.exists(cache):
        with np.load(cache) as z:
            return {k: z[k] for k in z.files}
    log("generating %d x %d events" % (K0, E))
    ev = synth.generate_events(np.arange(K0), E, seed=11)
    if cache:
        np.savez(cache, **ev)
    return ev


def c1_loop():
    """Config 1: main_file.py:38-46 over the committed 1,550-record log, once through the drop-in
    modules (GPU per-call kernels) and once through oracle/ekf_numpy.py (the NumPy restatement,
    bit-identical to the reference) on this host's CPU: microseconds per record."""
    import gzip
    import importlib
    import tempfile
    from oracle import ekf_numpy as npo
    golden = os.path.join(ROOT, "tests", "golden")
    with gzip.open(os.path.join(golden, "c1_log.txt.gz"), "rt") as fh:
        text = fh.read()
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as fh:
        fh.write(text)
    os.environ["PEKF_LOG_PATH"] = fh.name
    sys.path.insert(0, os.path.join(ROOT, "poseestimationkf_amd", "dropin"))
    ReadFile = importlib.import_module("ReadFile")
    EKF = importlib.import_module("ExtendedKalmanFilter")
    Wahba = importlib.import_module("Wahba")
    g = ReadFile.getData()
    os.unlink(fh.name)
    T = [t[0] for t in g.timestamp]
    n = len(g.acc_1)

    def dropin():
        w = Wahba.Wahba(g.acc_0, g.mag_0)
        k = EKF.KalmanFilter(T[0], g.mag_0, g.acc_0, 0.5)
        k.setQ(1)
        k.setR(0.1)
        X, P = np.asarray([1., 0., 0., 0.]), np.identity(4)
        for i in range(n):
            z, P, K = k.Prediction(g.gyro[i], T[i + 1], X, P)
            w.getQuarternion(g.acc_1[i], g.mag_1[i], 0.5, 0.5)
            X, P = k.Correction(g.mag_1[i], g.acc_1[i], z, P, K)
        return X

    def numpy_port():
        Q, R = np.identity(3), np.identity(4) * 0.1
        X, P, prev = np.asarray([1., 0., 0., 0.]), np.identity(4), T[0]
        a0, m0 = np.asarray(g.acc_0, float), np.asarray(g.mag_0, float)
        for i in range(n):
            z, P, K = npo.predict(np.asarray(g.gyro[i], float), T[i + 1] - prev, X, P, Q, R)
            prev = T[i + 1]
            npo.wahba_quat(a0, m0, np.asarray(g.acc_1[i], float), np.asarray(g.mag_1[i], float), 0.5, 0.5)
            X, P = npo.correct(np.asarray(g.mag_1[i], float), np.asarray(g.acc_1[i], float), z, P, K, a0, m0)
        return X

    out = {"records": n}
    for name, fn in (("dropin_gpu_us_per_record", dropin), ("numpy_port_cpu_us_per_record", numpy_port)):
        fn()
        t0 = time.perf_counter()
        X = fn()
        out[name] = (time.perf_counter() - t0) / n * 1e6
        out[name.replace("us_per_record", "final_X")] = X.tolist()
    return out


def percall_dev(s):
    """The per-call predict / correct kernels at n = 1M items on device pointers (stream s): what an A/B of
    two builds alternates (PEKF_LIB selects the build)."""
    res = {}
    n = 1 << 20
    rng = np.random.default_rng(0)
    X = rng.normal(size=(n, 4))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    bufs = {k: engine.DeviceBuffer(a.nbytes).upload(np.ascontiguousarray(a)) for k, a in dict(
        g=rng.normal(size=(n, 3)), dt=np.full(n, 1e7), X=X, P=np.tile(np.eye(4), (n, 1, 1)),
        Q=np.tile(np.eye(3), (n, 1, 1)), R=np.tile(np.eye(4) * 0.1, (n, 1, 1)), acc=X[:, :3].copy(),
        mag=X[:, 1:].copy(), a0=np.tile([0, 0, 1.0], (n, 1)), m0=np.tile([0.5, 0, -0.86], (n, 1))).items()}
    z, Pm, Kk, Xo, Po = (engine.DeviceBuffer(8 * n * k) for k in (4, 16, 16, 4, 16))
    b = bufs
    ms = timed(lambda: check(lib.pekf_predict_dev(n, b["g"].ptr, b["dt"].ptr, b["X"].ptr, b["P"].ptr, b["Q"].ptr,
                                                  b["R"].ptr, z.ptr, Pm.ptr, Kk.ptr, None, s)), s)
    byts = n * 8 * (3 + 1 + 4 + 16 + 9 + 16 + 4 + 16 + 16)
    res["predict_dev"] = {"n": n, "kernel_ms": ms, "items_per_s": n / (ms * 1e-3), "gbs": byts / (ms * 1e-3) / 1e9,
                          "hbm_frac": byts / (ms * 1e-3) / 1e9 / HBM}
    ms = timed(lambda: check(lib.pekf_correct_dev(n, b["mag"].ptr, b["acc"].ptr, z.ptr, Pm.ptr, Kk.ptr, b["a0"].ptr,
                                                  b["m0"].ptr, Xo.ptr, Po.ptr, s)), s)
    byts = n * 8 * (3 + 3 + 4 + 16 + 16 + 3 + 3 + 4 + 16)
    res["correct_dev"] = {"n": n, "kernel_ms": ms, "items_per_s": n / (ms * 1e-3), "gbs": byts / (ms * 1e-3) / 1e9,
                          "hbm_frac": byts / (ms * 1e-3) / 1e9 / HBM}
    log("per-call predict %.2f ms, correct %.2f ms at n=1M" % (res["predict_dev"]["kernel_ms"], ms))
    return res


def live_resume(s, K0=16384, E=1024, tile=64):
    """A live session fed in chunks (pekf_live_resume_dev) beside the one launch (pekf_live_ext_dev), 1,048,576
    filters x 1,024 events, FP64 records, for f32 and FP64 events: (a) the one launch, (b) the session in one
    chunk -- a same-box A B B A of the two -- then 8 chunks of 128, 64 of 16 and 341 of 3 plus one of 1.  Each
    case's time beside what its bytes predict: the state read and written per filter and launch at the HBM
    fraction pekf_state_layout_dev (k_state_layout, a pure state copy) reaches on the same box."""
    ev = bench_events(K0, E)
    K = K0 * tile
    init = np.tile(np.concatenate([ev["init_acc"], ev["init_mag"]], axis=1), (tile, 1))
    ib = engine.DeviceBuffer(init.nbytes).upload(init)
    tb = engine.DeviceBuffer(8 * K).upload(np.tile(ev["t_init"], tile).astype(np.int64))
    f = engine.BatchedEKF(K)
    cnt, refs = engine.DeviceBuffer(4 * K), engine.DeviceBuffer(48 * K)
    # the yardstick of a state-sized copy: AoS -> SoA of X, P (160 B read, 112 B written per filter)
    xs, ps = engine.DeviceBuffer(32 * K), engine.DeviceBuffer(80 * K)
    ms = timed(lambda: check(lib.pekf_state_layout_dev(K, f.X.ptr, f.P.ptr, xs.ptr, ps.ptr, 1, s)), s, reps=9)
    frac = K * 272 / (ms * 1e-3) / 1e9 / HBM
    res = {"filters": K, "events_per_filter": E, "state_layout": {"kernel_ms": ms, "bytes": K * 272, "hbm_frac": frac}}
    log("k_state_layout: %.3f ms, %.2f of HBM" % (ms, frac))
    del xs, ps
    cuts = {"b_1x1024": [E], "c_8x128": [128] * 8, "d_64x16": [16] * 64, "e_341x3+1": [3] * 341 + [1]}
    for form, flags, row in (("f32", 0, 16), ("f64", engine.EV_F64_EVENTS, 32)):
        src = synth.pack_events(ev) if form == "f32" else synth.pack_events64(ev, engine.server_event_values(ev))
        assert src.shape[0] == E and not (form == "f32" and synth.has_time_events(src))
        evb = engine.DeviceBuffer(E * K * row)
        for e0 in range(0, E, 64):   # tiled and uploaded 64 rows at a time
            blk = np.ascontiguousarray(np.tile(src[e0:e0 + 64], (1, tile, 1)))
            check(lib.pekf_memcpy_h2d(evb.ptr + e0 * K * row, blk.ctypes.data, blk.nbytes, None))
        del src, blk
        sb = int(lib.pekf_live_state_bytes(K, flags))
        state = engine.DeviceBuffer(sb)

        def one_launch():
            check(lib.pekf_live_ext_dev(K, E, evb.ptr, ib.ptr, tb.ptr, 0.1, f.X.ptr, f.P.ptr, f.q, f.r, cnt.ptr,
                                        refs.ptr, flags, None, s))

        def session(sizes):
            def run():
                e0 = 0
                for i, n in enumerate(sizes):
                    check(lib.pekf_live_resume_dev(K, n, evb.ptr + e0 * K * row, ib.ptr, tb.ptr, 0.1, f.X.ptr, f.P.ptr,
                                                   f.q, f.r, cnt.ptr, refs.ptr, flags, state.ptr, int(i > 0), None,
                                                   None, 0, None, s))
                    e0 += n
            return run
        out = {"state_bytes_per_filter": sb // K}
        abba = []
        for name, fn in (("a", one_launch), ("b", session(cuts["b_1x1024"])), ("b", session(cuts["b_1x1024"])),
                         ("a", one_launch)):
            f.reset(s)
            abba.append((name, timed(fn, s)))
        out["abba_ms"] = abba
        a_ms = float(np.mean([m for n, m in abba if n == "a"]))
        out["a_one_launch_ms"] = a_ms
        for name, sizes in cuts.items():
            f.reset(s)
            ms = timed(session(sizes), s)
            # the state written by every launch and read by every launch but the first
            byts = sb * (2 * len(sizes) - 1)
            pred = byts / (frac * HBM * 1e9) * 1e3
            out[name] = {"launches": len(sizes), "total_ms": ms, "ms_per_chunk": ms / len(sizes),
                         "extra_ms": ms - a_ms, "state_bytes": byts, "predicted_extra_ms": pred,
                         "unexplained_ms": ms - a_ms - pred,
                         "unexplained_us_per_launch": (ms - a_ms - pred) / len(sizes) * 1e3}
            log("%s events, %s: %.2f ms (%.3f per chunk), extra %.2f, predicted %.2f" %
                (form, name, ms, ms / len(sizes), ms - a_ms, pred))
        res[form] = out
        del evb, state
    res["device"] = engine.device_name(0)
    return res


def phone_session(s, K0=16384, E=1024, tile=64, n_avg=100):
    """Sessions fed from the phones' first message (pekf_frontend_init_resume_dev + pekf_live_join_dev per chunk)
    beside the route that needs phase 2 finished first (one pekf_frontend_init_ext_dev over the whole phase-2
    plane, then pekf_live_resume_dev on the phase-3 plane in the same chunks): 1,048,576 phones x 1,024 rows of
    FP64 events, phone k's first 600 + 8 (k % 8) rows in the phase-2 plane and the rest in the phase-3 plane
    (no-message events elsewhere), fed in 1, 8 and 64 chunks; a same-box A B B A per chunking.  The new route
    reads each phone's rows twice, once per plane, and zeroes the join state before every session (timed with
    it).  Then the phase-2 chunk launch alone beside what its bytes predict at the HBM fraction
    pekf_state_layout_dev (k_state_layout, a pure state copy) reaches on the same box."""
    ev = bench_events(K0, E)
    K, flags, row = K0 * tile, engine.EV_F64_EVENTS, 32
    cut = 600 + 8 * (np.arange(K0) % 8)
    in2 = np.arange(E)[:, None] < cut[None, :]
    vals = engine.server_event_values(ev)
    planes = []
    for keep in (in2, ~in2):
        src = synth.pack_events64(dict(ev, types=np.where(keep, ev["types"], synth.EV_NONE)), vals)
        buf = engine.DeviceBuffer(E * K * row)
        for e0 in range(0, E, 64):   # tiled and uploaded 64 rows at a time
            blk = np.ascontiguousarray(np.tile(src[e0:e0 + 64], (1, tile, 1)))
            check(lib.pekf_memcpy_h2d(buf.ptr + e0 * K * row, blk.ctypes.data, blk.nbytes, None))
        planes.append(buf)
        del src, blk
    ev2, ev3 = planes
    f = engine.BatchedEKF(K)
    tsb = engine.DeviceBuffer(8 * K).upload(np.tile(ev["t_init"], tile).astype(np.int64))
    ib, tb, rb = engine.DeviceBuffer(48 * K), engine.DeviceBuffer(8 * K), engine.DeviceBuffer(4 * K)
    cnt, refs = engine.DeviceBuffer(4 * K), engine.DeviceBuffer(48 * K)
    sb2, sb3 = int(lib.pekf_frontend_init_state_bytes(K, flags)), int(lib.pekf_live_state_bytes(K, flags))
    st2, st3 = engine.DeviceBuffer(sb2), engine.DeviceBuffer(sb3)
    xs, ps = engine.DeviceBuffer(32 * K), engine.DeviceBuffer(80 * K)
    ms = timed(lambda: check(lib.pekf_state_layout_dev(K, f.X.ptr, f.P.ptr, xs.ptr, ps.ptr, 1, s)), s, reps=9)
    frac = K * 272 / (ms * 1e-3) / 1e9 / HBM
    res = {"phones": K, "rows": E, "n_avg": n_avg, "phase2_state_bytes_per_phone": sb2 // K,
           "join_state_bytes_per_phone": sb3 // K,
           "state_layout": {"kernel_ms": ms, "bytes": K * 272, "hbm_frac": frac}}
    log("k_state_layout: %.3f ms, %.2f of HBM" % (ms, frac))
    del xs, ps

    def phase2_chunk(e0, n, resume):
        check(lib.pekf_frontend_init_resume_dev(K, n, ev2.ptr + e0 * K * row, tsb.ptr, n_avg, ib.ptr, tb.ptr, rb.ptr,
                                                flags, st2.ptr, resume, s))

    def parent_route(sizes):
        def run():
            check(lib.pekf_frontend_init_ext_dev(K, E, ev2.ptr, tsb.ptr, n_avg, ib.ptr, tb.ptr, None, rb.ptr, flags, s))
            e0 = 0
            for i, n in enumerate(sizes):
                check(lib.pekf_live_resume_dev(K, n, ev3.ptr + e0 * K * row, ib.ptr, tb.ptr, 0.1, f.X.ptr, f.P.ptr, f.q,
                                               f.r, cnt.ptr, refs.ptr, flags, st3.ptr, int(i > 0), None, None, 0, None,
                                               s))
                e0 += n
        return run

    def new_route(sizes):
        def run():
            check(lib.pekf_memset(st3.ptr, 0, sb3, s))
            e0 = 0
            for i, n in enumerate(sizes):
                phase2_chunk(e0, n, int(i > 0))
                check(lib.pekf_live_join_dev(K, n, ev3.ptr + e0 * K * row, ib.ptr, tb.ptr, 0.1, f.X.ptr, f.P.ptr, f.q,
                                             f.r, cnt.ptr, refs.ptr, flags, st3.ptr, None, None, 0, None, s))
                e0 += n
        return run

    final = {}
    for chunks in (1, 8, 64):
        sizes = [E // chunks] * chunks
        abba = []
        for name, fn in (("a", parent_route(sizes)), ("b", new_route(sizes)), ("b", new_route(sizes)),
                         ("a", parent_route(sizes))):
            f.reset(s)
            abba.append((name, timed(fn, s)))
        a_ms, b_ms = (float(np.mean([m for n, m in abba if n == which])) for which in "ab")
        # the same result either way: the last timed session ran on the state the repetitions before it left, so
        # compare the filters of one fresh session of each route
        for which, fn in (("a", parent_route(sizes)), ("b", new_route(sizes))):
            f.reset(s)
            fn()
            check(lib.pekf_stream_sync(s))
            final[which] = f.X.download((K, 4), np.float64)
        n = E // chunks
        # the phase-2 chunk launch alone (a middle chunk): n events, the state read and written, the outputs
        p2_ms = timed(lambda: phase2_chunk((chunks // 2) * n, n, 1), s, reps=9)
        p2_bytes = K * (n * row + 2 * (sb2 // K) + 48 + 8 + 4)
        res["chunks_%d" % chunks] = {
            "abba_ms": abba, "a_parent_route_ms": a_ms, "b_phone_session_ms": b_ms, "b_over_a": b_ms / a_ms,
            "b_ms_per_chunk": b_ms / chunks, "a_ms_per_chunk": a_ms / chunks, "same_final_X": bool(
                np.array_equal(final["a"], final["b"])),
            "phase2_chunk": {"kernel_ms": p2_ms, "bytes": p2_bytes, "predicted_ms": p2_bytes / (frac * HBM * 1e9) * 1e3,
                             "hbm_frac": p2_bytes / (p2_ms * 1e-3) / 1e9 / HBM}}
        log("%d chunks: parent route %.2f ms, phone session %.2f ms (%.3f per chunk); phase-2 chunk %.3f ms, "
            "predicted %.3f" % (chunks, a_ms, b_ms, b_ms / chunks, p2_ms, res["chunks_%d" % chunks]["phase2_chunk"][
                "predicted_ms"]))
    res["ready"] = int(rb.download((K,), np.int32).sum())
    res["device"] = engine.device_name(0)
    return res


def noise_per_filter(s, K0=16384, E=1024, tile=64):
    """Per-filter noise beside launch-wide noise, a same-box A B B A (a: the scalar kernel, b: the per-filter one)
    of (1) the multi-record launch at config 3's shape, 1,048,576 filters x 10,000 records over the 1,024-row
    window (pekf_run_dev against pekf_run_noise_dev) and (2) a live session of 1,048,576 filters x 1,024 f32
    events, FP64 records, as one chunk and as 64 chunks of 16 (pekf_live_resume_dev against
    pekf_live_resume_noise_dev).  The plane holds the four pairs the tests run at, dealt as b % 4; the scalar
    launches run at the first pair.  Leg c runs the per-filter kernels on a uniform plane (every lane the first
    pair), which tells the kernels' form from the data; the config-3 part also times the scalar launch with the
    compiler's own schedule (d) and at each of the four pairs.  24 B more are read per filter and launch."""
    pairs = np.array([(1.0, 0.1), (0.37, 2.5), (4.0, 0.01), (1e-3, 1.0)])
    B, W, N = 1 << 20, 1024, 10000
    res = {"pairs": pairs.tolist()}
    fa = engine.BatchedEKF(B)
    fb = engine.BatchedEKF(B, q=pairs[np.arange(B) % 4, 0], r=pairs[np.arange(B) % 4, 1])
    win = engine.IMUWindow(B, W).synthesize(stream=s)
    # two more legs tell the kernel's form from its schedule and from its data: c, the per-filter kernel on a
    # uniform plane (every lane the scalar launch's pair), and d, the scalar launch with the compiler's own
    # schedule (PEKF_RUN_PIN=0), which is the schedule the per-filter kernels over 40 B records have
    fc = engine.BatchedEKF(B, q=np.full(B, 1.0), r=np.full(B, 0.1))
    abba = []
    for name, f in (("a", fa), ("b", fb), ("c", fc), ("d", fa), ("d", fa), ("c", fc), ("b", fb), ("a", fa)):
        f.reset(s)
        if name == "d":
            os.environ["PEKF_RUN_PIN"] = "0"
        abba.append((name, timed(lambda: f.run_async(win, N, 0, s), s)))
        os.environ.pop("PEKF_RUN_PIN", None)
    a_ms, b_ms, c_ms, d_ms = (float(np.mean([m for n, m in abba if n == which])) for which in "abcd")
    res["run_config3"] = {"filters": B, "records": N, "window": W, "abba_ms": abba, "a_scalar_ms": a_ms,
                          "b_per_filter_ms": b_ms, "c_per_filter_uniform_plane_ms": c_ms, "d_scalar_no_pin_ms": d_ms,
                          "b_over_a": b_ms / a_ms, "c_over_a": c_ms / a_ms, "d_over_a": d_ms / a_ms,
                          "x_finite": bool(np.isfinite(fb.X.download((B, 4), np.float64)).all())}
    log("config 3 launch: scalar %.2f ms, per-filter %.2f ms, per-filter on a uniform plane %.2f ms, scalar without "
        "PIN %.2f ms (%s)" % (a_ms, b_ms, c_ms, d_ms, abba))
    # ... and the scalar launch at each of the other pairs: what the data alone costs
    per_pair = []
    for qp, rp in pairs:
        fp = engine.BatchedEKF(B, q=float(qp), r=float(rp))
        per_pair.append(timed(lambda: fp.run_async(win, N, 0, s), s))
        del fp
    res["run_config3"]["scalar_ms_at_each_pair"] = per_pair
    log("config 3 launch, scalar, at each pair: %s" % per_pair)
    del win

    ev = bench_events(K0, E)
    K, row = K0 * tile, 16
    assert K == B
    init = np.tile(np.concatenate([ev["init_acc"], ev["init_mag"]], axis=1), (tile, 1))
    ib = engine.DeviceBuffer(init.nbytes).upload(init)
    tb = engine.DeviceBuffer(8 * K).upload(np.tile(ev["t_init"], tile).astype(np.int64))
    cnt, refs = engine.DeviceBuffer(4 * K), engine.DeviceBuffer(48 * K)
    src = synth.pack_events(ev)
    assert src.shape[0] == E and not synth.has_time_events(src)
    evb = engine.DeviceBuffer(E * K * row)
    for e0 in range(0, E, 64):   # tiled and uploaded 64 rows at a time
        blk = np.ascontiguousarray(np.tile(src[e0:e0 + 64], (1, tile, 1)))
        check(lib.pekf_memcpy_h2d(evb.ptr + e0 * K * row, blk.ctypes.data, blk.nbytes, None))
    del src, blk
    state = engine.DeviceBuffer(int(lib.pekf_live_state_bytes(K, 0)))

    def session(f, sizes):
        entry, noise = ((lib.pekf_live_resume_dev, (f.q, f.r)) if f.noise is None else
                        (lib.pekf_live_resume_noise_dev, (f.noise.ptr,)))

        def run():
            e0 = 0
            for i, n in enumerate(sizes):
                check(entry(K, n, evb.ptr + e0 * K * row, ib.ptr, tb.ptr, 0.1, f.X.ptr, f.P.ptr, *noise, cnt.ptr,
                            refs.ptr, 0, state.ptr, int(i > 0), None, None, 0, None, s))
                e0 += n
        return run
    for name, sizes in (("live_1x1024", [E]), ("live_64x16", [16] * 64)):
        abba = []
        for which, f in (("a", fa), ("b", fb), ("c", fc), ("c", fc), ("b", fb), ("a", fa)):   # (c: a uniform plane)
            f.reset(s)
            abba.append((which, timed(session(f, sizes), s)))
        a_ms, b_ms, c_ms = (float(np.mean([m for n, m in abba if n == which])) for which in "abc")
        res[name] = {"filters": K, "events_per_filter": E, "launches": len(sizes), "abba_ms": abba,
                     "a_scalar_ms": a_ms, "b_per_filter_ms": b_ms, "c_per_filter_uniform_plane_ms": c_ms,
                     "b_over_a": b_ms / a_ms, "c_over_a": c_ms / a_ms,
                     "extra_us_per_launch": (b_ms - a_ms) / len(sizes) * 1e3,
                     "uniform_extra_us_per_launch": (c_ms - a_ms) / len(sizes) * 1e3,
                     "x_finite": bool(np.isfinite(fb.X.download((K, 4), np.float64)).all())}
        log("%s: scalar %.3f ms, per-filter %.3f ms, per-filter on a uniform plane %.3f ms (%s)" %
            (name, a_ms, b_ms, c_ms, abba))
    res["device"] = engine.device_name(0)
    return res


def session_move(s, K0=16384, rows=16, tile=64, n_avg=20):
    """Moving live phones (pekf_session_export_dev / pekf_session_import_dev) beside the only route there was,
    snapshot + restore through the host.  An engine.PhoneSession of K0 * tile phones (FP64 events), started by one
    `rows`-row chunk of every plane, with n_cal = 100 and without phase 1:
      export_<n> / import_<n>   one launch each on n listed columns -- 1, 1,024 scattered, every column -- the
                  import back into the columns the pack came from (idempotent, so repeats time the same work);
      snapshot_restore          wall time of session.snapshot() + PhoneSession.restore on new filters, once.
    Then what a compaction buys: the session's launches for a `rows`-row chunk when only every 16th column holds a
    live phone (the others recycled, their rows empty), against a session of K / 16 columns that adopted those
    phones (export_columns + import_columns) fed the same phones' rows.  Nothing is asserted about the times."""
    from poseestimationkf_amd._lib import EV_F64_EVENTS
    K, row = K0 * tile, 32 * K0 * tile
    ev = synth.generate_events(np.arange(K0), 3 * rows, seed=12)

    def tiled(planes, t):   # host FP64 planes (E, k0, 4) -> a device buffer [E][k0 * t] double4, each row tiled
        E, k0 = planes.shape[:2]
        src, dst = engine.DeviceBuffer(planes.nbytes).upload(planes), engine.DeviceBuffer(planes.nbytes * t)
        for e in range(E):
            for i in range(t):
                check(lib.pekf_memcpy_d2d(dst.ptr + 32 * k0 * (e * t + i), src.ptr + 32 * k0 * e, 32 * k0, s))
        check(lib.pekf_stream_sync(s))
        return dst

    def chunk_of(sess, evb):
        k, f, r = sess.batch, sess.filters, 32 * sess.batch * rows
        ev1, ev2, ev3 = evb.ptr, evb.ptr + r, evb.ptr + 2 * r

        def chunk():
            if sess.n_cal is not None:
                check(lib.pekf_magcal_resume_dev(k, rows, ev1, sess.n_cal, sess._cal.ptr, sess._fit.ptr, sess._status.ptr,
                                                 EV_F64_EVENTS, sess._p1state.ptr, 1, s))
                for p in (ev2, ev3):
                    check(lib.pekf_magcal_apply_dev(k, rows, p, sess._cal.ptr, sess._status.ptr, EV_F64_EVENTS, s))
            check(lib.pekf_frontend_init_resume_dev(k, rows, ev2, sess._t_start.ptr, sess.n_avg, sess._init.ptr,
                                                    sess._t_init.ptr, sess._ready.ptr, EV_F64_EVENTS, sess._p2state.ptr,
                                                    1, s))
            check(lib.pekf_live_join_dev(k, rows, ev3, sess._init.ptr, sess._t_init.ptr, sess.alpha, f.X.ptr, f.P.ptr,
                                         f.q, f.r, sess._cnt.ptr, sess._refs.ptr, EV_F64_EVENTS, sess._state.ptr, None,
                                         None, 0, None, s))
        return chunk

    host = synth.pack_events64(ev, ev["values"].astype(np.float64))
    evb = tiled(host, tile)
    rng = np.random.default_rng(3)
    lists = {"1": np.array([K // 3], np.int32), "1024": rng.choice(K, min(1024, K), replace=False).astype(np.int32),
             "all": np.arange(K, dtype=np.int32)}
    res = {"phones": K, "rows_per_plane": rows}
    for n_cal in (100, None):
        sess = engine.PhoneSession(engine.BatchedEKF(K), n_avg=n_avg, n_cal=n_cal)
        sess.feed_planes(evb, rows, evb, rows, offset2=row * rows, offset3=row * 2 * rows,
                         **(dict(planes1=evb, n1=rows) if n_cal else {}))
        groups = sess._move_groups()
        f, p2, p1 = groups[0], groups[1], groups[2] or (None, 0, None, None, None)
        per_col = int(lib.pekf_session_columns_bytes(1, n_cal or 0, EV_F64_EVENTS))
        out = {"n_cal": n_cal, "pack_bytes_per_column": per_col,
               "state_bytes_per_phone": (sess._p2state.nbytes + sess._state.nbytes +
                                         (sess._p1state.nbytes if n_cal else 0)) // K}
        for name, cols in lists.items():
            n = len(cols)
            dev = engine.DeviceBuffer(cols.nbytes).upload(cols)
            pack = engine.DeviceBuffer(per_col * n)

            def move(entry, dev=dev, n=n, pack=pack):
                return lambda: check(entry(K, n, dev.ptr, EV_F64_EVENTS, *f, *p2, *p1, pack.ptr, s))
            e1, i1, i2, e2 = (timed(move(lib.pekf_session_export_dev), s, reps=9),
                              timed(move(lib.pekf_session_import_dev), s, reps=9),
                              timed(move(lib.pekf_session_import_dev), s, reps=9),
                              timed(move(lib.pekf_session_export_dev), s, reps=9))
            byts = 2 * n * per_col + 4 * n       # each launch reads and writes the columns' bytes once
            out["move_" + name] = {"columns": n, "export_ms": [e1, e2], "import_ms": [i1, i2], "bytes_per_launch": byts,
                                   "export_gbs": byts / (min(e1, e2) * 1e-3) / 1e9,
                                   "import_gbs": byts / (min(i1, i2) * 1e-3) / 1e9,
                                   "bytes_predict_ms": byts / (HBM * 1e9) * 1e3}
            log("n_cal=%s, %s columns (%d): export %.4f / %.4f ms, import %.4f / %.4f ms; the bytes predict %.4f ms"
                % (n_cal, name, n, e1, e2, i1, i2, out["move_" + name]["bytes_predict_ms"]))
            del pack, dev
        t0 = time.perf_counter()
        snap = sess.snapshot()
        t1 = time.perf_counter()
        again = engine.PhoneSession.restore(engine.BatchedEKF(K), snap)
        check(lib.pekf_device_sync())
        t2 = time.perf_counter()
        out["snapshot_restore"] = {"snapshot_ms": (t1 - t0) * 1e3, "restore_ms": (t2 - t1) * 1e3,
                                   "host_bytes": int(sum(v.nbytes for v in snap.values() if isinstance(v, np.ndarray)))}
        log("n_cal=%s: snapshot %.0f ms + restore %.0f ms through the host (%.2f GB)"
            % (n_cal, (t1 - t0) * 1e3, (t2 - t1) * 1e3, out["snapshot_restore"]["host_bytes"] / 1e9))
        del snap, again
        res["n_cal_100" if n_cal else "no_phase1"] = out
        if n_cal is None:
            break
        # ---- what a compaction buys (the calibrating session): every 16th column stays live
        live = np.arange(0, K, 16, dtype=np.int32)
        gone = np.setdiff1d(np.arange(K, dtype=np.int32), live)
        full_ms = timed(chunk_of(sess, evb), s, reps=9)
        sess.recycle(gone)
        sparse_host = host.copy()
        none = np.array([0, 0, 0, synth.EV64_NONE_W], np.uint64).view(np.float64)   # the FP64 no-message event
        sparse_host[:, np.arange(K0) % 16 != 0] = none
        evs = tiled(sparse_host, tile)
        sparse_ms = [timed(chunk_of(sess, evs), s, reps=9)]
        t0 = time.perf_counter()
        small = engine.PhoneSession(engine.BatchedEKF(len(live)), n_avg=n_avg, n_cal=n_cal)
        small.import_columns(np.arange(len(live)), sess.export_columns(live))
        adopt_ms = (time.perf_counter() - t0) * 1e3
        evl = tiled(np.ascontiguousarray(host[:, ::16]), tile)
        small_ms = [timed(chunk_of(small, evl), s, reps=9)]
        empty_ms = timed(chunk_of(sess, evs), s, reps=9)            # (now every column of it is free)
        small_ms.append(timed(chunk_of(small, evl), s, reps=9))
        sess.import_columns(live, small.export_columns(np.arange(len(live)), release=False))   # ... and live again
        sparse_ms.append(timed(chunk_of(sess, evs), s, reps=9))
        res["compaction"] = {"n_cal": n_cal, "columns": K, "live_phones": len(live), "full_session_chunk_ms": full_ms,
                             "sparse_session_chunk_ms": sparse_ms, "compact_session_chunk_ms": small_ms,
                             "emptied_session_chunk_ms": empty_ms, "adopt_wall_ms": adopt_ms,
                             "live_total_counts": int(small.total_counts.sum())}
        log("a %d-row chunk: %.3f ms with every column live, %s ms with %d of %d live, %s ms in a %d-column session "
            "that adopted them (export + import, host side included: %.1f ms)"
            % (rows, full_ms, sparse_ms, len(live), K, small_ms, len(live), adopt_ms))
        del small, evs, evl, sess
    res["device"] = engine.device_name(0)
    return res


def main():
    st = engine.Stream()
    s = st.handle
    res = {}
    if os.environ.get("PEKF_AUX_ONLY") == "session_move":
        print(json.dumps({"session_move": session_move(s, tile=int(os.environ.get("PEKF_AUX_TILE", "64")))}))
        return
    if os.environ.get("PEKF_AUX_ONLY") == "noise_per_filter":
        print(json.dumps({"noise_per_filter": noise_per_filter(s)}))
        return
    if os.environ.get("PEKF_AUX_ONLY") == "live_resume":
        print(json.dumps({"live_resume": live_resume(s)}))
        return
    if os.environ.get("PEKF_AUX_ONLY") == "phone_session":
        print(json.dumps({"phone_session": phone_session(s)}))
        return

    # ---- front-end: 16K generated event streams tiled x64 -> 1,048,576 filters x 1,024 events
    K0, E, tile = 16384, 1024, 64
    ev = bench_events(K0, E)
    planes = np.ascontiguousarray(np.tile(synth.pack_events(ev), (1, tile, 1)))
    K = K0 * tile
    init = np.tile(np.concatenate([ev["init_acc"], ev["init_mag"]], axis=1), (tile, 1))
    tinit = np.tile(ev["t_init"], tile)
    evb = engine.DeviceBuffer(planes.nbytes).upload(planes)
    del planes
    ib = engine.DeviceBuffer(init.nbytes).upload(init)
    tb = engine.DeviceBuffer(tinit.nbytes).upload(tinit.astype(np.int64))
    r_max = E // 3 + 1
    win = engine.IMUWindow(K, r_max)
    cnt = engine.DeviceBuffer(4 * K)
    err = engine.DeviceBuffer(4).upload(np.zeros(1, np.int32))
    ms = timed(lambda: check(lib.pekf_frontend_dev(K, E, evb.ptr, ib.ptr, tb.ptr, 0.1, r_max, win.gd.ptr,
                                                   win.am.ptr, win.my.ptr, cnt.ptr, win.refs.ptr, err.ptr, s)), s)
    counts = cnt.download((K,), np.int32)
    recs = int(counts.sum())
    byts = K * E * 16 + recs * 40
    res["frontend"] = {"filters": K, "events_per_filter": E, "records": recs, "kernel_ms": ms,
                       "events_per_s": K * E / (ms * 1e-3), "gbs": byts / (ms * 1e-3) / 1e9,
                       "hbm_frac": byts / (ms * 1e-3) / 1e9 / HBM, "bytes": byts}
    log("frontend: %.2f ms, %.2e events/s, %.0f GB/s" % (ms, K * E / (ms * 1e-3), byts / (ms * 1e-3) / 1e9))
    # phase 2 on the same event planes: two passes (the means, then the variances of the first 100
    # samples of each type; the second pass stops once every type has had its 100)
    ib2, tb2, sb2, rb2 = (engine.DeviceBuffer(k * K) for k in (48, 8, 96, 4))
    ms = timed(lambda: check(lib.pekf_frontend_init_dev(K, E, evb.ptr, tb.ptr, 100, ib2.ptr, tb2.ptr, sb2.ptr,
                                                        rb2.ptr, s)), s)
    # algorithmic bytes: pass 1 reads every event; pass 2 a filter's events up to the one that brings
    # its last sensor type to 100 samples
    ty = ev["types"]
    last = np.zeros(K0, np.int64)
    for t in (synth.EV_ACC, synth.EV_GYRO, synth.EV_MAG):
        c = np.cumsum(ty == t, axis=0)
        last = np.maximum(last, np.argmax(c >= 100, axis=0) + 1)
    byts = 16 * (K * E + tile * int(last.sum()))
    res["frontend_init"] = {"filters": K, "events_per_filter": E, "kernel_ms": ms, "events_per_s": K * E / (ms * 1e-3),
                            "ready": int(rb2.download((K,), np.int32).sum()), "bytes": byts,
                            "gbs": byts / (ms * 1e-3) / 1e9, "hbm_frac": byts / (ms * 1e-3) / 1e9 / HBM}
    log("frontend phase 2: %.2f ms" % ms)
    # the means alone (stats = NULL, as engine.run_session asks): pass 1 only
    ms = timed(lambda: check(lib.pekf_frontend_init_dev(K, E, evb.ptr, tb.ptr, 100, ib2.ptr, tb2.ptr, None,
                                                        rb2.ptr, s)), s)
    byts = 16 * K * E
    res["frontend_init_means"] = {"filters": K, "events_per_filter": E, "kernel_ms": ms,
                                  "events_per_s": K * E / (ms * 1e-3), "bytes": byts,
                                  "gbs": byts / (ms * 1e-3) / 1e9, "hbm_frac": byts / (ms * 1e-3) / 1e9 / HBM}
    log("frontend phase 2, means only: %.2f ms" % ms)
    del ib2, tb2, sb2, rb2
    # the filter over the front-end's records (split pipeline, second half): one multi-record launch
    # with counts, as engine.BatchedEKF.run does for a front-end window
    n_rec = int(counts.max())
    f = engine.BatchedEKF(K)
    ms_run = timed(lambda: f.run_async(win, n_rec, 0, s, None, cnt), s)
    del f
    res["frontend_then_filter"] = {"filters": K, "records": recs, "frontend_ms": res["frontend"]["kernel_ms"],
                                   "filter_ms": ms_run, "total_ms": res["frontend"]["kernel_ms"] + ms_run}
    log("split pipeline: front-end %.2f + filter %.2f ms" % (res["frontend"]["kernel_ms"], ms_run))
    del win
    # the same events -> filter in one launch (pekf_live_dev): 16 B read per event, the state
    # (160 B per filter) read and written once
    f = engine.BatchedEKF(K)
    cnt2, refs2 = engine.DeviceBuffer(4 * K), engine.DeviceBuffer(48 * K)
    ms = timed(lambda: f.run_events_async(evb, E, ib, tb, cnt2, refs2, 0.1, s), s)
    assert np.array_equal(cnt2.download((K,), np.int32), counts)
    byts = K * E * 16 + K * (160 + 160 + 48 + 48 + 8 + 4)
    res["live"] = {"filters": K, "events_per_filter": E, "records": recs, "kernel_ms": ms,
                   "events_per_s": K * E / (ms * 1e-3), "records_per_s": recs / (ms * 1e-3), "bytes": byts,
                   "gbs": byts / (ms * 1e-3) / 1e9, "hbm_frac": byts / (ms * 1e-3) / 1e9 / HBM,
                   "vs_split": res["frontend_then_filter"]["total_ms"] / ms}
    log("fused front-end + filter: %.2f ms (split %.2f ms)" % (ms, res["frontend_then_filter"]["total_ms"]))
    del f, cnt2, refs2, evb
    if os.environ.get("PEKF_AUX_ONLY") == "live":
        print(json.dumps(res))
        return

    # ---- side outputs on a config-3-sized window
    B, W, N = 1 << 20, 1024, 10000
    win = engine.IMUWindow(B, W).synthesize(stream=s)
    q = engine.DeviceBuffer(32 * B).upload(np.tile([1.0, 0, 0, 0], (B, 1)))
    ms = timed(lambda: check(lib.pekf_gyro_chain_dev(B, N, W, 0, win.gd.ptr, q.ptr, None, s)), s)
    res["gyro_chain"] = {"filters": B, "records": N, "kernel_ms": ms, "steps_per_s": B * N / (ms * 1e-3),
                         "gbs": B * N * 16 / (ms * 1e-3) / 1e9, "hbm_frac": B * N * 16 / (ms * 1e-3) / 1e9 / HBM}
    log("gyro chain: %.1f ms" % ms)
    Nw = 1024
    out = engine.DeviceBuffer(32 * B * Nw)
    ms = timed(lambda: check(lib.pekf_wahba_stream_dev(B, Nw, W, 0, win.am.ptr, win.my.ptr, win.refs.ptr, 0.5, 0.5,
                                                       out.ptr, s)), s)
    res["wahba_stream"] = {"filters": B, "records": Nw, "kernel_ms": ms, "quats_per_s": B * Nw / (ms * 1e-3),
                           "gbs": B * Nw * 56 / (ms * 1e-3) / 1e9, "hbm_frac": B * Nw * 56 / (ms * 1e-3) / 1e9 / HBM}
    log("wahba stream: %.1f ms" % ms)
    del win, out
    if os.environ.get("PEKF_AUX_ONLY") == "side":
        print(json.dumps(res))
        return

    # ---- online serving: every launch advances 1M filters by ONE new record; the state X, P and
    # the reference vectors are read and the state written through HBM each launch.  AoS: 40 B
    # record + 48 B refs + 32+128 B state read (P's cache lines come whole) + 32+128 B written;
    # SoA (X[4][B], P[10][B]): 40 + 48 + 32+80 + 32+80 B.
    B1 = 1 << 20
    win1 = engine.IMUWindow(B1, 8).synthesize(stream=s)
    for layout, per in (("aos", 40 + 48 + 32 + 128 + 32 + 128), ("soa", 40 + 48 + 32 + 80 + 32 + 80)):
        f1 = engine.BatchedEKF(B1, layout=layout)
        k = [0]

        def one_step():
            f1.run_async(win1, 1, k[0] % 8, s)
            k[0] += 1
        ms = timed(one_step, s, reps=20)
        res["online_step_" + layout] = {
            "filters": B1, "records_per_launch": 1, "kernel_ms": ms, "steps_per_s": B1 / (ms * 1e-3),
            "bytes_per_filter_step": per, "gbs": B1 * per / (ms * 1e-3) / 1e9,
            "hbm_frac": B1 * per / (ms * 1e-3) / 1e9 / HBM}
        log("online step %s (1M filters x 1 record): %.3f ms" % (layout, ms))
        del f1
    del win1

    # ---- filter handle: one FP64 record per filter per pekf_filter_update_dev (device pointers).
    # Bytes: gyro/acc/mag 72 + t 8 + prev_t 8+8 + refs 48 + state (AoS 32+128 / SoA 32+80) read and
    # written + X_out 32.
    rng = np.random.default_rng(3)
    a0 = rng.normal(size=(B1, 3))
    m0 = rng.normal(size=(B1, 3))
    ub = {k: engine.DeviceBuffer(8 * B1 * w).upload(np.ascontiguousarray(rng.normal(size=(B1, w)) if w == 3 else
                                                                          np.full((B1, 1), 10_000_000, np.int64)))
          for k, w in (("g", 3), ("a", 3), ("m", 3), ("t", 1))}
    xo = engine.DeviceBuffer(32 * B1)
    for layout, st_b in (("aos", 2 * (32 + 128)), ("soa", 2 * (32 + 80))):
        h = engine.FilterHandle(a0, m0, layout=layout)
        per = 72 + 8 + 16 + 48 + st_b + 32
        ms = timed(lambda: check(lib.pekf_filter_update_dev(h.h, ub["g"].ptr, ub["t"].ptr, ub["a"].ptr, ub["m"].ptr,
                                                            None, xo.ptr, s)), s, reps=20)
        res["handle_update_" + layout] = {
            "filters": B1, "kernel_ms": ms, "updates_per_s": B1 / (ms * 1e-3), "bytes_per_filter": per,
            "gbs": B1 * per / (ms * 1e-3) / 1e9, "hbm_frac": B1 * per / (ms * 1e-3) / 1e9 / HBM}
        log("handle update %s (1M filters, FP64 records): %.3f ms" % (layout, ms))
        del h
    del ub, xo
    # the same update from HOST arrays (pekf_filter_update: records in over PCIe through the pinned
    # staging buffer, X out): the PCIe-inclusive rate of the host-buffer boundary (never the headline)
    hg, ha, hm = (np.ascontiguousarray(rng.normal(size=(B1, 3))) for _ in range(3))
    h = engine.FilterHandle(a0, m0, layout="soa")
    for i in range(13):
        if i == 3:
            t0 = time.perf_counter()
        xh = h.update(hg, np.full(B1, 10_000_000 * (i + 1), np.int64), ha, hm)
    ms = (time.perf_counter() - t0) / 10 * 1e3
    res["handle_update_host_soa"] = {"filters": B1, "wall_ms": ms, "updates_per_s": B1 / (ms * 1e-3),
                                     "pcie_bytes_per_filter": 80 + 32,
                                     "pcie_gbs": B1 * 112 / (ms * 1e-3) / 1e9, "x_finite": bool(np.isfinite(xh).all())}
    log("handle update from host arrays (1M filters, PCIe-inclusive): %.3f ms" % ms)
    del h

    # ---- per-call operators at n = 1M (device pointers)
    res.update(percall_dev(s))

    # ---- per-call latency at n = 1 (host pointers): the ctypes engine wrappers, and the CPython
    # binding the drop-in KalmanFilter.Prediction / Correction use (what main_file.py pays per call)
    from poseestimationkf_amd import _fastcall
    gy, X1, P1, Q1, R1 = [0.1, 0.2, 0.3], np.array([1.0, 0, 0, 0]), np.eye(4), np.eye(3), np.eye(4) * 0.1
    mg, ac, a0, m0 = [0.5, 0, -0.86], [0, 0.1, 0.99], [0, 0, 1.0], [0.5, 0, -0.86]
    for key, pred, corr in (("ctypes_call_us", engine.predict, engine.correct),
                            ("dropin_call_us", _fastcall.predict, _fastcall.correct)):
        lat = {"predict": [], "correct": []}
        for i in range(300):
            t0 = time.perf_counter()
            zz, pm, kk = pred(gy, 1e7, X1, P1, Q1, R1)
            t1 = time.perf_counter()
            corr(mg, ac, zz, pm, kk, a0, m0)
            t2 = time.perf_counter()
            if i >= 50:
                lat["predict"].append(t1 - t0)
                lat["correct"].append(t2 - t1)
        res[key] = {k: float(np.median(v) * 1e6) for k, v in lat.items()}
        log("%s: %s" % (key, res[key]))
    res["c1_loop"] = c1_loop()
    log("config-1 loop: %s" % res["c1_loop"])
    res["device"] = engine.device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
