"""Host side of the batched engine: device buffers, resident IMU windows, fused runs.

Everything here is plumbing around the C ABI (include/pekf.h); all arithmetic of the
filter runs in the HIP kernels of libpekf.so.
"""
from __future__ import annotations

import copy
import ctypes
import os
import types

import numpy as np

from . import synth
from ._lib import (EV_F32_RECORDS, EV_F64_EVENTS, EV_TIME_EVENTS, RUN_MIXED_PRECISION, RUN_STATE_SOA, WIRE_FRAME_ROWS,
                   check, dptr, f64, lib)


# ------------------------------------------------------------------ device plumbing

class DeviceBuffer:
    """A raw hipMalloc allocation owned by Python."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self._lib = lib   # freed by the library that allocated it
        p = ctypes.c_void_p()
        check(lib.pekf_malloc(ctypes.byref(p), max(1, self.nbytes)))
        self.ptr = p.value

    def upload(self, arr, stream=None):
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes, (a.nbytes, self.nbytes)
        check(lib.pekf_memcpy_h2d(self.ptr, a.ctypes.data, a.nbytes, stream))
        return self

    def download(self, shape, dtype, stream=None, offset=0):
        out = np.empty(shape, dtype)
        assert offset + out.nbytes <= self.nbytes
        check(lib.pekf_memcpy_d2h(out.ctypes.data, self.ptr + offset, out.nbytes, stream))
        return out

    def free(self):
        if getattr(self, "ptr", None):
            self._lib.pekf_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Stream:
    def __init__(self):
        self._lib = lib
        s = ctypes.c_void_p()
        check(lib.pekf_stream_create(ctypes.byref(s)))
        self.handle = s.value

    def sync(self):
        check(self._lib.pekf_stream_sync(self.handle))

    def __del__(self):
        try:
            if self.handle:
                self._lib.pekf_stream_destroy(self.handle)
        except Exception:
            pass


class Event:
    def __init__(self):
        self._lib = lib
        e = ctypes.c_void_p()
        check(lib.pekf_event_create(ctypes.byref(e)))
        self.handle = e.value

    def record(self, stream=None):
        check(lib.pekf_event_record(self.handle, stream))

    def sync(self):
        check(lib.pekf_event_sync(self.handle))

    def elapsed_ms(self, end):
        ms = ctypes.c_float()
        check(lib.pekf_event_elapsed_ms(ctypes.byref(ms), self.handle, end.handle))
        return ms.value

    def __del__(self):
        try:
            if self.handle:
                self._lib.pekf_event_destroy(self.handle)
        except Exception:
            pass


def set_device(dev):
    check(lib.pekf_set_device(int(dev)))


def device_name(dev=0):
    buf = ctypes.create_string_buffer(128)
    check(lib.pekf_device_name(int(dev), buf, 128))
    return buf.value.decode()


PERCALL_SERVICE, PERCALL_LAUNCH = 0, 1


def percall_mode(mode=None):
    """How n = 1 per-call operators reach the GPU (include/pekf.h): PERCALL_SERVICE (a resident
    kernel answering requests in pinned host memory, the default) or PERCALL_LAUNCH (one launch
    per call).  Sets the mode when given; returns the mode in effect."""
    if mode is not None:
        check(lib.pekf_set_percall_mode(int(mode)))
    m = ctypes.c_int()
    check(lib.pekf_get_percall_mode(ctypes.byref(m)))
    return m.value


# ------------------------------------------------------------------ recorded traces (host ingest)

def read_log_records(path):
    """Parse one server log natively (pekf_log_scan / pekf_log_read) into a 1-filter synth.Records.

    The records are the 40 B stream format: f32 sensor values, u32 ns dt (the drop-in
    ReadFile / logformat path keeps the parsed float64 values instead)."""
    bpath = os.fsencode(path)
    n = ctypes.c_int64()
    check(lib.pekf_log_scan(bpath, ctypes.byref(n)))
    n = n.value
    gyro, acc, mag = (np.empty((n, 1, 3), np.float32) for _ in range(3))
    dtw = np.empty((n, 1), np.uint32)
    dtx = np.empty((n, 1), np.float64)
    acc0, mag0, t0, n_esc = np.empty((1, 3)), np.empty((1, 3)), ctypes.c_double(), ctypes.c_int64()
    check(lib.pekf_log_read_ext(bpath, n, gyro.ctypes.data, acc.ctypes.data, mag.ctypes.data, dtw.ctypes.data,
                                dtx.ctypes.data, ctypes.byref(n_esc), dptr(acc0), dptr(mag0), ctypes.byref(t0)))
    # records whose T - previousT does not fit the dt word (a pause >= 2^31 ns, a negative or fractional
    # difference) carry it in the float64 side plane
    return synth.Records(gyro, acc, mag, dtw, acc0, mag0, dtx if n_esc.value else None)


# ------------------------------------------------------------------ resident IMU window

def _stack_ragged(cols, lens, n_records=None):
    """Filters of different lengths side by side: cols[k] (lens[k], ...) -> ((n, K, ...) zero-padded, counts (K,)
    int32 each filter's own rows), n the longest or n_records."""
    n = int(max(lens)) if n_records is None else int(n_records)
    out = np.zeros((n, len(cols)) + cols[0].shape[1:], cols[0].dtype)
    for k, c in enumerate(cols):
        m = min(n, c.shape[0])
        out[:m, k] = c[:m]
    return out, np.minimum(np.asarray(lens, np.int64), n).astype(np.int32)


class _RecordWindow:
    """What the two resident windows share: `window` steps x `batch` filters as three planes [window][batch] of
    4 / 4 / 2 scalars of _DTYPE (gd, am, my; filter-minor), the per-filter reference block refs (batch, 6)
    float64, the ragged counts, and the side outputs of the entries _WAHBA / _GYRO."""
    _DTYPE = _WAHBA = _GYRO = None

    def __init__(self, batch, window):
        self.batch, self.window = int(batch), int(window)
        n = self.batch * self.window * np.dtype(self._DTYPE).itemsize
        self.gd = DeviceBuffer(4 * n)
        self.am = DeviceBuffer(4 * n)
        self.my = DeviceBuffer(2 * n)
        self.refs = DeviceBuffer(48 * self.batch)
        self.counts = None  # per-filter valid record counts when filters are ragged (logs, front-end)

    @property
    def nbytes(self):
        return self.gd.nbytes + self.am.nbytes + self.my.nbytes

    def _dtx_arg(self):
        """the entry's dt side plane argument, for the window that has one"""
        return ()

    def _download(self, cols):
        """(gd, am, my, refs) of filter columns `cols`"""
        gd, am, my = (b.download((self.window, self.batch, k), self._DTYPE)[:, cols]
                      for b, k in ((self.gd, 4), (self.am, 4), (self.my, 2)))
        return gd, am, my, self.refs.download((self.batch, 6), np.float64)[cols]

    def wahba_quaternions(self, n_steps=None, step0=0, k_acc=0.5, k_mag=0.5):
        """Pure-Wahba attitude of every record with fixed weights (main_file.py:40): (n_steps, batch, 4)."""
        n_steps = self.window if n_steps is None else int(n_steps)
        out = DeviceBuffer(32 * n_steps * self.batch)
        check(getattr(lib, self._WAHBA)(self.batch, n_steps, self.window, int(step0), self.am.ptr, self.my.ptr,
                                        self.refs.ptr, float(k_acc), float(k_mag), out.ptr, None))
        check(lib.pekf_device_sync())
        return out.download((n_steps, self.batch, 4), np.float64)

    def gyro_chain(self, q0=None, n_steps=None, step0=0, want_traj=False):
        """Pure-gyro attitude (RK4 of the gyro records alone, KFS/KalmanFilter.cpp:149) from q0 (default
        [1,0,0,0]); returns (q_final (batch,4), traj (n_steps,batch,4) or None)."""
        n_steps = self.window if n_steps is None else int(n_steps)
        q = np.tile([1.0, 0.0, 0.0, 0.0], (self.batch, 1)) if q0 is None else f64(q0, (self.batch, 4))
        qb = DeviceBuffer(32 * self.batch).upload(q)
        tb = DeviceBuffer(32 * n_steps * self.batch) if want_traj else None
        check(getattr(lib, self._GYRO)(self.batch, n_steps, self.window, int(step0), self.gd.ptr, *self._dtx_arg(),
                                       qb.ptr, tb.ptr if tb is not None else None, None))
        check(lib.pekf_device_sync())
        return (qb.download((self.batch, 4), np.float64),
                tb.download((n_steps, self.batch, 4), np.float64) if want_traj else None)


class IMUWindow(_RecordWindow):
    """`window` steps x `batch` filters of the 40 B/step input record, resident in HBM.

    Planes (filter-minor, see synth.pack_planes): gd float4, am float4, my float2, plus the
    per-filter reference block refs (batch, 6) float64.  Either uploaded from host records or
    generated on the device with the bit-identical Philox generator (pekf_synth_dev).
    """
    _DTYPE, _WAHBA, _GYRO = np.float32, "pekf_wahba_stream_dev", "pekf_gyro_chain_ext_dev"

    def __init__(self, batch, window):
        super().__init__(batch, window)
        self.dtx = None     # dt side plane [window][batch] float64 when some record's dt is escaped (pekf.h)

    def _dtx_arg(self):
        # escaped records (a dt the word cannot hold) take their dt from the side plane, as in the filter
        return (self.dtx.ptr if self.dtx is not None else None,)

    @classmethod
    def from_records(cls, rec: synth.Records):
        return cls.from_planes(*synth.pack_planes(rec), rec.acc0, rec.mag0, rec.dtx)

    @classmethod
    def from_planes(cls, gd, am, my, acc0, mag0, dtx=None):
        W, K = gd.shape[:2]
        win = cls(K, W)
        win.gd.upload(np.ascontiguousarray(gd, np.float32))
        win.am.upload(np.ascontiguousarray(am, np.float32))
        win.my.upload(np.ascontiguousarray(my, np.float32))
        win.refs.upload(synth.refs_array(acc0, mag0))
        if dtx is not None:
            win.dtx = DeviceBuffer(8 * W * K).upload(np.ascontiguousarray(dtx, np.float64))
        return win

    @classmethod
    def from_logs(cls, paths, n_records=None):
        """One filter per server log, parsed natively (pekf_log_read).

        Logs may differ in length: the window holds the longest log's records (n_records caps
        it), shorter logs are zero-padded and win.counts[b] is filter b's own record count,
        which BatchedEKF.run applies so each filter consumes exactly its own records."""
        recs = [read_log_records(p) for p in paths]
        lens = [r.dtw.shape[0] for r in recs]

        def cat(name):  # logs without escapes get a zero side plane (never read: their words are not escapes)
            cols = [getattr(r, name) if getattr(r, name) is not None else np.zeros(r.dtw.shape) for r in recs]
            return _stack_ragged([c[:, 0] for c in cols], lens, n_records)
        dtx = cat("dtx")[0] if any(r.dtx is not None for r in recs) else None
        dtw, counts = cat("dtw")
        rec = synth.Records(cat("gyro")[0], cat("acc")[0], cat("mag")[0], dtw,
                            np.concatenate([r.acc0 for r in recs]), np.concatenate([r.mag0 for r in recs]), dtx)
        win = cls.from_records(rec)
        win.counts = counts
        return win

    def synthesize(self, seed=synth.DEFAULT_SEED, first_filter=0, missing=False,
                   params=synth.SynthParams(), stream=None):
        sc = np.array(params.scales(), dtype=np.float64)
        check(lib.pekf_synth_dev(self.batch, self.window, int(first_filter), int(seed) & 0xFFFFFFFF,
                                 1 if missing else 0, dptr(sc), float(params.ar_w), self.gd.ptr,
                                 self.am.ptr, self.my.ptr, self.refs.ptr, stream))
        if stream is None:
            check(lib.pekf_device_sync())
        return self

    def download_filters(self, cols):
        """Pull the records of filter columns `cols` back to the host as synth.Records."""
        cols = np.asarray(cols)
        gd, am, my, refs = self._download(cols)
        dtx = None if self.dtx is None else self.dtx.download((self.window, self.batch), np.float64)[:, cols]
        return synth.unpack_planes(gd, am, my, refs[:, :3], refs[:, 3:], dtx)


class RecordWindow64(_RecordWindow):
    """`window` steps x `batch` filters of FP64 records (80 B per filter-record, pekf_run_rec64_dev), for
    inputs that are float64 to begin with: recorded logs, parsed into float64 as the reference parses
    them (ReadFile.py:14-21), where IMUWindow's 40 B record would round them to f32.

    Planes [window][batch]: gd double4 {gyro xyz, dt_ns}, am double4 {acc xyz, mag x}, my double2
    {mag yz}; dt is the float64 T - previousT itself (any pause, clock step or fraction).  Every record
    is a full record (no missing-magnetometer flag).  BatchedEKF.run / run_async take it like an
    IMUWindow (FP64 AoS state)."""
    _DTYPE, _WAHBA, _GYRO = np.float64, "pekf_wahba_stream_rec64_dev", "pekf_gyro_chain_rec64_dev"

    @classmethod
    def from_arrays(cls, gyro, dt_ns, acc, mag, acc0, mag0):
        """gyro / acc / mag (W, K, 3), dt_ns (W, K) float64 (the reference's T - previousT); acc0 / mag0
        (K, 3) the reference pairs (KalmanFilter(T0, mag_0, acc_0))."""
        gyro, acc, mag = (np.asarray(a, np.float64) for a in (gyro, acc, mag))
        W, K = gyro.shape[:2]
        dt = np.asarray(dt_ns, np.float64).reshape(W, K)
        win = cls(K, W)
        win.gd.upload(np.ascontiguousarray(np.concatenate([gyro, dt[..., None]], axis=2)))
        win.am.upload(np.ascontiguousarray(np.concatenate([acc, mag[..., :1]], axis=2)))
        win.my.upload(np.ascontiguousarray(mag[..., 1:]))
        win.refs.upload(synth.refs_array(np.asarray(acc0, np.float64).reshape(K, 3),
                                         np.asarray(mag0, np.float64).reshape(K, 3)))
        return win

    @classmethod
    def from_logs(cls, paths, n_records=None):
        """One filter per server log, parsed natively into float64 (pekf_log_read64); ragged logs as
        IMUWindow.from_logs (zero-padded, win.counts = each filter's own record count)."""
        cols = []
        for p in paths:
            bpath = os.fsencode(p)
            n = ctypes.c_int64()
            check(lib.pekf_log_scan(bpath, ctypes.byref(n)))
            g, a, m = (np.empty((n.value, 3)) for _ in range(3))
            dt = np.empty(n.value)
            a0, m0, t0 = np.empty(3), np.empty(3), ctypes.c_double()
            check(lib.pekf_log_read64(bpath, n.value, g.ctypes.data, a.ctypes.data, m.ctypes.data, dt.ctypes.data,
                                      dptr(a0), dptr(m0), ctypes.byref(t0)))
            cols.append((g, dt, a, m, a0, m0))
        lens = [c[1].shape[0] for c in cols]
        (g, counts), (dt, _), (a, _), (m, _) = (_stack_ragged([c[i] for c in cols], lens, n_records) for i in range(4))
        win = cls.from_arrays(g, dt, a, m, np.stack([c[4] for c in cols]), np.stack([c[5] for c in cols]))
        win.counts = counts
        return win

    def download_filters(self, cols):
        """The records of filter columns `cols` as float64 arrays: (gyro (W, n, 3), dt_ns (W, n), acc (W, n, 3),
        mag (W, n, 3), refs (n, 6))."""
        gd, am, my, refs = self._download(np.asarray(cols))
        return gd[..., :3], gd[..., 3], am[..., :3], np.concatenate([am[..., 3:4], my], axis=-1), refs


# ------------------------------------------------------------------ server front-end (raw events)

EVENT_FORMS = ("f32", "f64")


def server_event_values(ev):
    """The sample values the server computes with: ev["values64"] when the events came as wire text
    (wire.events_from_wire: the server's own std::stod parse), else the doubles it would parse from
    the phone's Float.toString of ev["values"] (wire.server_values)."""
    from . import wire
    return np.asarray(ev["values64"], np.float64) if "values64" in ev else wire.server_values(ev["values"])


def _event_planes(ev, events="f32"):
    """(device event planes, n_events, flags).  events="f32": synth.pack_events (16 B, the float32
    samples; time events inserted for gaps the 30-bit field cannot hold), flags = PEKF_EV_TIME_EVENTS when
    the planes hold any.  events="f64": synth.pack_events64 of the server's values (32 B,
    server_event_values), flags = PEKF_EV_F64_EVENTS."""
    if events not in EVENT_FORMS:
        raise ValueError("events must be 'f32' or 'f64'")
    if events == "f64":
        planes = synth.pack_events64(ev, server_event_values(ev))
        return DeviceBuffer(planes.nbytes).upload(planes), planes.shape[0], EV_F64_EVENTS
    planes = synth.pack_events(ev)
    return (DeviceBuffer(planes.nbytes).upload(planes), planes.shape[0],
            EV_TIME_EVENTS if synth.has_time_events(planes) else 0)


def run_frontend(ev, alpha=0.1, r_max=None, events="f32"):
    """Raw phone events (synth.generate_events layout) -> (window of records, counts (K,) int32).

    Runs pekf_frontend_ext_dev.  Every record needs a gyro, an accelerometer and a
    magnetometer event, so r_max defaults to n_events // 3 + 1.  Raises if a filter overflows r_max.
    events="f32": float32 samples -> an IMUWindow of 40 B records; event gaps of any size go through
    time events, and records whose dt does not fit the dt word through the window's dt side plane
    (win.dtx, kept only if some record needed it).  events="f64": the server's own sample values
    (server_event_values) -> a RecordWindow64 of FP64 records, every field FP64 (pekf_run_rec64_dev's
    input), any dt."""
    K = np.asarray(ev["types"]).shape[1]
    E0 = np.asarray(ev["types"]).shape[0]
    evb, E, flags = _event_planes(ev, events)
    r_max = E0 // 3 + 1 if r_max is None else int(r_max)
    init = DeviceBuffer(48 * K).upload(np.concatenate([ev["init_acc"], ev["init_mag"]], axis=1).astype(np.float64))
    tib = DeviceBuffer(8 * K).upload(np.ascontiguousarray(ev["t_init"], np.int64))
    cnt = DeviceBuffer(4 * K)
    errb = DeviceBuffer(4)
    win = (RecordWindow64 if events == "f64" else IMUWindow)(K, max(1, r_max))
    dtx = None
    while True:
        # without a side plane first; only if some record's dt does not fit the dt word (err bit 1: a
        # pause of 2^31 ns or more; never with FP64 events, whose records hold any dt) run again with one
        # (8 B per record slot, kept in win.dtx)
        errb.upload(np.zeros(1, np.int32))
        check(lib.pekf_frontend_ext_dev(K, E, evb.ptr, init.ptr, tib.ptr, float(alpha), r_max, win.gd.ptr,
                                        win.am.ptr, win.my.ptr, dtx.ptr if dtx is not None else None, cnt.ptr,
                                        win.refs.ptr, flags, errb.ptr, None))
        check(lib.pekf_device_sync())
        err = int(errb.download((1,), np.int32)[0])
        if err & 1 and dtx is None and events != "f64":
            dtx = DeviceBuffer(8 * K * max(1, r_max))
            continue
        break
    if err & 2:
        raise ValueError("more than r_max=%d records for some filter" % r_max)
    if err & 4:
        win.dtx = dtx
    win.counts = cnt.download((K,), np.int32)
    return win, win.counts


def frontend_init(ev, n_avg=100, stats=True, events="f32"):
    """Phase-2 events (synth.generate_events layout; ev["t_init"] = the time before the first one) ->
    dict(init (K, 6) raw {acc, mag} means, t_init (K,) int64, ready (K,) bool, gyro_mean (K, 3),
    var_acc / var_mag / var_gyro (K, 3)) by pekf_frontend_init_ext_dev: the inputs run_frontend needs
    for phase 3 (KFS/Parser.cpp:36-58,84-140, KFS/InitialValues.cpp).  stats=False: init / t_init /
    ready only (the kernel then skips its second pass, the variances).  events: as run_frontend ("f64":
    the statistics of the server's own sample values)."""
    K = np.asarray(ev["types"]).shape[1]
    evb, E, flags = _event_planes(ev, events)   # phase 2 always honours time events
    tsb = DeviceBuffer(8 * K).upload(np.ascontiguousarray(ev["t_init"], np.int64))
    p2 = _launch_phase2(K, E, evb.ptr, tsb, n_avg, flags, stats=stats)
    check(lib.pekf_device_sync())
    out = dict(init=p2.init.download((K, 6), np.float64), t_init=p2.t_init.download((K,), np.int64),
               ready=p2.ready.download((K,), np.int32).astype(bool))
    if stats:
        st = p2.stats.download((K, 12), np.float64)
        out.update(gyro_mean=st[:, 0:3], var_acc=st[:, 3:6], var_mag=st[:, 6:9], var_gyro=st[:, 9:12])
    return out


def _launch_phase2(K, E, ev_ptr, t_start, n_avg, flags, stream=None, stats=False):
    """pekf_frontend_init_ext_dev on the first E rows of device event planes (enqueued) -> its outputs as
    DeviceBuffers: init (K, 6), t_init (K,) int64, ready (K,) int32 and, when asked for, stats (K, 12)."""
    out = types.SimpleNamespace(init=DeviceBuffer(48 * K), t_init=DeviceBuffer(8 * K), ready=DeviceBuffer(4 * K),
                                stats=DeviceBuffer(96 * K) if stats else None)
    check(lib.pekf_frontend_init_ext_dev(K, int(E), ev_ptr, t_start.ptr, int(n_avg), out.init.ptr, out.t_init.ptr,
                                         out.stats.ptr if stats else None, out.ready.ptr, flags & EV_F64_EVENTS,
                                         stream))
    return out


def calibrate_magnetometer(ev, n_cal=100, events="f32"):
    """Phase-1 events (synth.generate_calibration_events layout, or wire.events_from_wire(..., phase=1)) ->
    each phone's magnetometer calibration by pekf_magcal_dev (KFS/Magnetometer_Calibration.cpp): dict(bias
    (K, 3), W (K, 3, 3), fit (K, 6) the quadric {a, b, c, d, e, f}, status (K,) int32 (include/pekf.h: 0
    calibrated, 1 n_cal or fewer messages, 2 the samples determine no quadric, 3 not an ellipsoid),
    calibrated (K,) bool, cal / status_dev the device buffers run_session / run_wire_session take).  A phone
    that is not calibrated has bias 0, W = I and fit NaN, and its samples are left as they are.
    events: as run_frontend."""
    K = np.asarray(ev["types"]).shape[1]
    if "t_init" not in ev:
        ev = dict(ev, t_init=np.zeros(K, np.int64))
    evb, E, flags = _event_planes(ev, events)
    dev = _launch_calibration(K, E, evb.ptr, n_cal, flags, None)
    check(lib.pekf_device_sync())
    return _calibration_result(K, dev)


def _launch_calibration(K, E, ptr, n_cal, flags, stream):
    """pekf_magcal_dev on the first E rows of device event planes (enqueued) -> dict(cal, fit_dev, status_dev)
    DeviceBuffers: what pekf_magcal_apply_dev reads, and what _calibration_result downloads after a sync."""
    cal, fit, st = DeviceBuffer(96 * K), DeviceBuffer(48 * K), DeviceBuffer(4 * K)
    check(lib.pekf_magcal_dev(K, int(E), ptr, int(n_cal), cal.ptr, fit.ptr, st.ptr, flags & EV_F64_EVENTS, stream))
    return dict(cal=cal, fit_dev=fit, status_dev=st)


def _calibration_result(K, dev):
    """calibrate_magnetometer's dict from _launch_calibration's buffers (the launch has completed)."""
    c = dev["cal"].download((K, 12), np.float64)
    status = dev["status_dev"].download((K,), np.int32)
    return dict(bias=c[:, :3].copy(), W=c[:, 3:].reshape(K, 3, 3).copy(),
                fit=dev["fit_dev"].download((K, 6), np.float64), status=status, calibrated=status == 0,
                cal=dev["cal"], status_dev=dev["status_dev"])


def _apply_calibration(calibration, batch, n_events, ev_ptr, flags, stream=None):
    """pekf_magcal_apply_dev on device event planes (enqueued): the magnetometer events of the calibrated
    phones become W (m - bias).  calibration: calibrate_magnetometer's dict, or _launch_calibration's (of the
    session's own phones, its status still on the device)."""
    if "status" in calibration and len(calibration["status"]) != batch:
        raise ValueError("the calibration is of %d phones, the session of %d" % (len(calibration["status"]), batch))
    check(lib.pekf_magcal_apply_dev(batch, int(n_events), ev_ptr, calibration["cal"].ptr,
                                    calibration["status_dev"].ptr, flags & EV_F64_EVENTS, stream))


def _record_flags(records, events="f32"):
    """pekf_live_ext_dev's record precision: "f64" (the low-pass acc / mag as the server's filter gets them,
    KFS/KalmanFilter.cpp:279-303) or "f32" (the 40 B stream record, as the split pipeline's).  FP64 events
    always make FP64 records."""
    if records not in ("f64", "f32"):
        raise ValueError("records must be 'f64' or 'f32'")
    if events == "f64" and records != "f64":
        raise ValueError("FP64 events make FP64 records (records='f64')")
    return EV_F32_RECORDS if records == "f32" else 0


def trajectory_rows(trajectory, n_events):
    """The sessions' trajectory argument as a row count: False / None 0 (no trajectory), True n_events // 3
    (a record needs a gyro, an acc and a mag event after the previous one, so no filter has more), an int that
    many rows (records past them are applied and counted, not stored)."""
    if trajectory is None or trajectory is False:
        return 0
    if trajectory is True:
        return int(n_events) // 3
    rows = int(trajectory)
    if rows < 0 or rows >= 1 << 31:
        raise ValueError("trajectory must be True, False or a row count in [0, 2^31)")
    return rows


def record_times_ns(t_init, record_dt_ns):
    """The records' times: t_init (K,) plus the running sum of record_dt_ns (R, K) down each column, in
    float64 on the host (the server's T of each record, ExtendedKalmanFilter.py:62,67); the rows a filter
    did not write (NaN dt) and every row after them are NaN."""
    dt = np.asarray(record_dt_ns, np.float64)
    return np.asarray(t_init, np.float64)[None, :] + np.cumsum(dt, axis=0)


class _Trajectory:
    """The device buffers of a session's per-record output (pekf_live_traj_dev's traj / traj_dt), every byte
    0xFF so that what the kernel does not write reads as NaN; rows == 0: nothing is allocated."""

    def __init__(self, trajectory, n_events, batch, stream=None):
        self.rows, self.batch = trajectory_rows(trajectory, n_events), batch
        self.wanted = trajectory is not None and trajectory is not False   # (a cap of 0 rows: the empty result)
        self.traj = self.dt = None
        if self.rows:
            self.traj, self.dt = DeviceBuffer(32 * self.rows * batch), DeviceBuffer(8 * self.rows * batch)
            check(lib.pekf_memset(self.traj.ptr, 0xFF, self.traj.nbytes, stream))
            check(lib.pekf_memset(self.dt.ptr, 0xFF, self.dt.nbytes, stream))

    def result(self, t_init):
        """dict(trajectory (R, K, 4), record_dt_ns (R, K), record_times_ns (R, K)), after the launch's sync"""
        R, K = self.rows, self.batch
        if R:
            tr, dt = self.traj.download((R, K, 4), np.float64), self.dt.download((R, K), np.float64)
        else:
            tr, dt = np.empty((0, K, 4)), np.empty((0, K))
        return dict(trajectory=tr, record_dt_ns=dt, record_times_ns=record_times_ns(t_init, dt))


def _chunk_records(rows, batch):
    """The device planes a chunk fed with records=True exports its records into (pekf_live_resume_rec_dev's
    rec_gd / rec_am / rec_my): a RecordWindow64 of `rows` rows, every byte 0xFF as _Trajectory's buffers, so
    that what the kernel does not write reads as NaN."""
    win = RecordWindow64(batch, rows)
    if rows:
        for plane in (win.gd, win.am, win.my):
            check(lib.pekf_memset(plane.ptr, 0xFF, plane.nbytes, None))
    return win


def _scalar_noise_only(filters, what, session):
    """Refuses a per-filter-noise filter in a one-launch session, naming the chunked session to feed instead"""
    if getattr(filters, "noise", None) is not None:
        raise ValueError("%s runs the one-launch live kernels, which take one q and one r for the batch: feed a "
                         "per-filter-noise BatchedEKF through %s instead (one chunk gives the same launch)"
                         % (what, session))


def _run_live(filters, ev_planes, n_events, init, t_init, alpha, flags, trajectory, stream=None):
    """The fused launch every session ends in, run to completion: filters.run_events_async on device event
    planes and phase-2 results, with the trajectory buffers `trajectory` asks for -> (counts, refs DeviceBuffers,
    the _Trajectory)."""
    K = filters.batch
    cnt, refs = DeviceBuffer(4 * K), DeviceBuffer(48 * K)
    tj = _Trajectory(trajectory, n_events, K, stream)
    filters.run_events_async(ev_planes, n_events, init, t_init, cnt, refs, alpha, stream, flags=flags, traj=tj.traj,
                             traj_dt=tj.dt, traj_rows=tj.rows)
    check(lib.pekf_device_sync() if stream is None else lib.pekf_stream_sync(stream))
    return cnt, refs, tj


def _finish_session(filters, ev3, E3, p2, alpha, flags, trajectory, calibration, stream=None, from_frames=False):
    """Phase 3 + the filter on phase 2's results (_launch_phase2's) and the dict run_session documents.
    from_frames: calibration is _launch_calibration's, downloaded into the dict as calibration."""
    K = filters.batch
    cnt, refs, tj = _run_live(filters, ev3, E3, p2.init, p2.t_init, alpha, flags, trajectory, stream)
    out = dict(ready=p2.ready.download((K,), np.int32).astype(bool), counts=cnt.download((K,), np.int32),
               refs=refs.download((K, 6), np.float64))
    if tj.wanted:
        out.update(tj.result(p2.t_init.download((K,), np.int64)))
    if from_frames:
        calibration = out["calibration"] = _calibration_result(K, calibration)
    if calibration is not None:
        out["calibrated"] = np.asarray(calibration["calibrated"], bool).copy()
    return out


def run_session(phase2, phase3, filters, n_avg=100, alpha=0.1, records="f64", events="f32", calibration=None,
                trajectory=False):
    """A whole client session of the server on the device (KFS/Parser.cpp:28-72): phase-2 events ->
    initial means and start time (pekf_frontend_init_dev) -> phase-3 events -> records -> the filters'
    state (pekf_live_dev), the phase-2 results handed over in device memory.  phase3's times continue
    phase2's (its first gap is taken from phase2's last event, the time phase 3 starts from).
    filters: a BatchedEKF (FP64, AoS) whose state is advanced; records and events as
    BatchedEKF.run_events.
    calibration: calibrate_magnetometer's dict (phase 1): the magnetometer samples of both phases are
    corrected on the device first (pekf_magcal_apply_dev; the server's CorrectValues call sites,
    KFS/Parser.cpp:107,239), and the returned dict has calibrated (K,) bool.  None: no correction, no launch.
    Returns dict(ready (K,) bool -- a filter
    that never finished phase 2 has NaN references, applies no record and keeps its state --, counts
    (K,) records applied, refs (K, 6)).
    trajectory: True or a row cap R (True: phase 3's events // 3, which no filter exceeds) adds a pose per
    record, from the same launch (pekf_live_traj_dev): trajectory (R, K, 4) -- row r of filter k is its X
    after its own r-th record, the server's X_k --, record_dt_ns (R, K) the dt it was applied with and
    record_times_ns (R, K) its time (record_times_ns()); NaN from row counts[k] on."""
    K = filters.batch
    _scalar_noise_only(filters, "run_session", "PhoneSession")
    assert np.asarray(phase2["types"]).shape[1] == K and np.asarray(phase2["types"]).shape[0] > 0
    assert np.asarray(phase3["types"]).shape[1] == K
    t_last = np.asarray(phase2["times"], np.int64)[-1]
    ev2, E2, flags2 = _event_planes(phase2, events)
    ev3, E3, flags3 = _event_planes(dict(phase3, t_init=t_last), events)
    tsb = DeviceBuffer(8 * K).upload(np.ascontiguousarray(phase2["t_init"], np.int64))
    if calibration is not None:
        _apply_calibration(calibration, K, E2, ev2.ptr, flags2)
        _apply_calibration(calibration, K, E3, ev3.ptr, flags3)
    p2 = _launch_phase2(K, E2, ev2.ptr, tsb, n_avg, flags2)
    return _finish_session(filters, ev3, E3, p2, alpha, flags3 | _record_flags(records, events), trajectory,
                           calibration)


def _frames_shape(frames):
    """(n_frames, phones) of wire_events' frames, a host array or a (DeviceBuffer, n_frames, batch) triple."""
    if isinstance(frames, tuple):
        return int(frames[1]), int(frames[2])
    shape = np.shape(frames)
    if len(shape) != 3 or shape[2] != 100:
        raise ValueError("frames must be [n_frames][batch][100] bytes")
    return int(shape[0]), int(shape[1])


REFUSED_MODES = ("raise", "repair")


def _check_refused(refused):
    if refused not in REFUSED_MODES:
        raise ValueError("refused must be 'raise' or 'repair', not %r" % (refused,))


# pekf_wire_patch_col (include/pekf.h): one record per patched column
_PATCH_COL = np.dtype([("col", np.int32), ("bad_frame", np.int32), ("n", np.int32, 3), ("from_row", np.int32, 3),
                       ("n_cells", np.int32, 3), ("reserved", np.int32), ("first_t2", np.int64)])
assert _PATCH_COL.itemsize == 56
_EV64_TIME_LIMIT = 2.0 ** 51   # ns: what an FP64 event's time can hold (pekf_wire_dev.hip, take())


def _refused_frames(frames, F, K, cols, f0, stream):
    """The frames [f0, F) of the columns cols as (len(cols), F - f0, 100) uint8 on the host: a slice of a host
    array; for a device triple one gather launch (pekf_wire_gather_frames_dev) and one download of those frames."""
    n, nf = len(cols), F - f0
    if not isinstance(frames, tuple):
        return np.ascontiguousarray(np.asarray(frames, np.uint8)[f0:, cols].transpose(1, 0, 2))
    if n == 0 or nf == 0:
        return np.zeros((n, nf, 100), np.uint8)
    dcols = DeviceBuffer(4 * n).upload(np.ascontiguousarray(cols, np.int32), stream)
    out = DeviceBuffer(100 * n * nf)
    check(lib.pekf_wire_gather_frames_dev(K, F, frames[0].ptr, n, dcols.ptr, f0, out.ptr, stream))
    return out.download((n, nf, 100), np.uint8, stream)


def _repair_wire(w, dev, frames, F, K, stream, frame_rows, phase1, bad, bounds, dead):
    """wire_events' repair: the host takes over the phones the device parser stopped (bad (K,) >= 0) and blanks the
    columns of `dead` ((K,) bool or None: a session's phones that stopped in an earlier chunk).  The refused phones'
    frames from their bad_frame on are read by wire.parse_frames and walked as the kernel walks them (take(),
    pekf_wire_dev.hip): a frame the server skips is no message; a processed one is a message of its phase's plane
    (phases other than 1 / 2 / 3, or phase 1 without its plane, are skipped; a phase-1 time the event cannot hold
    is stored as 0); a frame the server's std::stod / std::stoll throw on, or a phase-2 / phase-3 time of 2^51 ns
    or more, stops the phone for good.  One pekf_wire_patch_dev launch writes the columns (dev: the parse's n1 /
    n2 / n3 / bad_frame DeviceBuffers, n1's None without phase 1); w's counts and row bounds are set afresh.
    Returns (bad_frame (K,) int32, repaired (K,) bool)."""
    from . import wire
    dead = np.zeros(K, bool) if dead is None else dead
    live = np.nonzero((bad >= 0) & ~dead)[0]
    cols = np.concatenate([live, np.nonzero(dead)[0]]).astype(np.int32)
    planes = ((1, 2, 3) if phase1 else (2, 3))
    counts = {1: w.get("n1"), 2: w["n2"], 3: w["n3"]}
    first_t2 = w["first_t2"].download((K,), np.int64, stream)
    rec = np.zeros(len(cols), _PATCH_COL)
    rec["col"], rec["bad_frame"] = cols, -1
    out_bad, repaired = np.full(K, -1, np.int32), np.zeros(K, bool)
    nl = len(live)
    f0 = int(bad[live].min()) if nl else F
    fills = []
    if nl:
        sub = _refused_frames(frames, F, K, live, f0, stream)
        p = wire.parse_frames(sub.reshape(-1, 100))
        st, ph = p["status"].reshape(nl, F - f0), p["phase"].reshape(nl, F - f0)
        ty, t = p["types"].reshape(nl, F - f0), p["times"].reshape(nl, F - f0)
        frame = f0 + np.arange(F - f0)[None, :]
        mine = frame >= bad[live][:, None]                     # the frames the device did not take
        td = t.astype(np.float64)
        fits = np.abs(td) < _EV64_TIME_LIMIT
        stops = mine & ((st == wire.THROWS) | ((st == wire.MESSAGE) & ((ph == 2) | (ph == 3)) & ~fits))
        stop = np.where(stops.any(axis=1), stops.argmax(axis=1), F - f0)
        taken = mine & (np.arange(F - f0)[None, :] < stop[:, None])
        out_bad[live] = np.where(stop < F - f0, f0 + stop, -1)
        repaired[live] = out_bad[live] != bad[live]
        rec["bad_frame"][:nl] = out_bad[live]
        # the events {x, y, z, bits(t) | type}: type 3 for a Type no sensor takes, a phase-1 time out of range as 0
        cell = np.empty((nl, F - f0, 4), np.uint64)
        cell[..., :3] = p["values"].reshape(nl, F - f0, 3).view(np.uint64)
        cell[..., 3] = np.where(fits, td, 0.0).view(np.uint64) | np.where(ty <= 2, ty, 3).astype(np.uint64)
        for pl in planes:
            msg = taken & (st == wire.MESSAGE) & (ph == pl)
            ii, jj = np.nonzero(msg)
            n_before = counts[pl][live]
            if frame_rows:   # row f; the rows between the phone's messages are no-message rows
                from_row = bad[live]
                at = f0 + jj - from_row[ii]
                n_cells = np.zeros(nl, np.int64)
                np.maximum.at(n_cells, ii, at + 1)
            else:            # the phone's next compacted rows
                from_row = n_before
                at = np.cumsum(msg, axis=1)[ii, jj] - 1
                n_cells = msg.sum(axis=1)
            rec["from_row"][:nl, pl - 1], rec["n_cells"][:nl, pl - 1] = from_row, n_cells
            rec["n"][:nl, pl - 1] = n_before + msg.sum(axis=1)
            if pl == 2:      # t_start: the first phase-2 message's time, if the phone had none before
                has = msg.any(axis=1) & (n_before == 0)
                t_first = t[np.arange(nl), msg.argmax(axis=1)]
                rec["first_t2"][:nl] = np.where(has, t_first, first_t2[live])
            fills.append((pl - 1, at, ii, cell[ii, jj]))
    cell_rows = int(rec["n_cells"].max(initial=0))
    cells = np.zeros((3, cell_rows, len(cols), 4), np.uint64)
    cells[..., 3] = np.uint64(synth.EV64_NONE_W)
    for pl, at, ii, e in fills:
        cells[pl, at, ii] = e
    cb = DeviceBuffer(max(cells.nbytes, 16))
    if cells.nbytes:
        cb.upload(cells, stream)
    n1b, n2b, n3b, badb = dev
    ev1, n1p = (w["ev1"].ptr, n1b.ptr) if phase1 else (None, None)
    rb = DeviceBuffer(max(rec.nbytes, 8))
    if rec.nbytes:
        rb.upload(rec, stream)
    check(lib.pekf_wire_patch_dev(K, len(cols), rec.ctypes.data, rb.ptr, cell_rows, cb.ptr if cell_rows else None,
                                  F if phase1 else 0, F, F, ev1, w["ev2"].ptr, w["ev3"].ptr, w["first_t2"].ptr, n1p,
                                  n2b.ptr, n3b.ptr, badb.ptr, F if frame_rows else 0,
                                  bounds.ptr if frame_rows else None, stream))
    check(lib.pekf_device_sync() if stream is None else lib.pekf_stream_sync(stream))
    for pl in planes:
        counts[pl][cols] = rec["n"][:, pl - 1]
    if frame_rows:
        bw = bounds.download((3,), np.int32)
        E2, E3, E1 = int(bw[0]), int(bw[1]), int(bw[2])
    else:
        E2, E3 = int(w["n2"].max(initial=0)), int(w["n3"].max(initial=0))
        E1 = int(w["n1"].max(initial=0)) if phase1 else 0
    w.update(E2=E2, E3=E3, ev3_from=F - E3 if frame_rows else 0)
    if phase1:
        w["E1"] = E1
    return out_bad, repaired


def wire_events(frames, stream=None, frame_rows=False, phase1=False, refused="raise", stopped=None):
    """The clients' 100-byte wire frames -> FP64 event planes on the device (pekf_wire_events_ext_dev;
    phase1: pekf_wire_events_p1_dev).

    frames: [n_frames][batch][100] uint8 (wire.frames) as a host array or a (DeviceBuffer, n_frames,
    batch) triple.  Returns dict(ev2, ev3 DeviceBuffers [n_frames][batch] double4, E2 / E3 the rows a
    consumer needs -- the most messages any phone has in phase 2 / 3, or with frame_rows n_frames --,
    n2 / n3 (batch,) int32 messages per phase, first_t2 DeviceBuffer (batch,) int64 (phase 2's t_start);
    with frame_rows, ev2's first E2 rows and ev3's E3 rows from row ev3_from hold every message).
    frame_rows (PEKF_WIRE_FRAME_ROWS): row f of each plane is frame f's message of that phase or the
    no-message event (for phones whose rows would drift apart; the consumers skip those rows).
    phase1: the phase-1 messages too, every one whatever its Type (calibrate_magnetometer's samples) -- the
    dict also has ev1 DeviceBuffer [n_frames][batch] double4, E1 the rows that hold them (ev1's first E1:
    the most phase-1 messages of any phone, or with frame_rows 1 + the last row holding one) and n1
    (batch,) int32; everything else is as without it, bit for bit.
    refused: what a frame the device parser does not take does.  "raise" (default): raises ValueError
    if a phone's frame is not in the client's form (wire.parse on the host reads any form std::stod
    does).  "repair": only that phone is affected, as with the server, which runs a process per client.  The launches
    are the same; if the error word reports a refused frame, the host reads the refused phones' frames from the
    earliest refused frame of any of them on
    (wire.parse_frames; for a device triple after one gather launch and a download of those phones' frames alone)
    and one patch launch (pekf_wire_patch_dev) writes their columns: a form std::stod reads (blanks, "+1.5", "7",
    hex, more than 19 digits, "inf") is the message the server parses, bit for bit; a frame its std::stod /
    std::stoll throw on, or a phase-2 / phase-3 time of 2^51 ns or more, which the event cannot carry, stops that
    phone there for good -- the reference has no try, so that client's server process ends, and nobody else's.  The
    dict then also has bad_frame (batch,) int32 -- -1, or the frame that stopped the phone -- and repaired (batch,)
    bool: the phone had at least one frame taken by the host.
    stopped ((batch,) bool or None): session plumbing, not a user option -- PhoneSession.feed_frames passes its
    own mark here: phones whose stream ended before these frames -- their columns
    are no-message rows whatever the frames hold (the same patch launch, with no cells), their bad_frame is -1."""
    _check_refused(refused)
    F, K = _frames_shape(frames)
    if isinstance(frames, tuple):
        fb = frames[0]
    else:
        fr = np.ascontiguousarray(frames, np.uint8)
        fb = DeviceBuffer(max(fr.nbytes, 4)).upload(fr)
    ev2, ev3 = DeviceBuffer(32 * max(F, 1) * K), DeviceBuffer(32 * max(F, 1) * K)
    t2b, n2b, n3b, badb = DeviceBuffer(8 * K), DeviceBuffer(4 * K), DeviceBuffer(4 * K), DeviceBuffer(4 * K)
    errb = DeviceBuffer(4).upload(np.zeros(1, np.int32))
    bounds = DeviceBuffer(12)
    if phase1:
        ev1, n1b = DeviceBuffer(32 * max(F, 1) * K), DeviceBuffer(4 * K)
        check(lib.pekf_wire_events_p1_dev(K, F, fb.ptr, F, F, F, ev1.ptr, ev2.ptr, ev3.ptr, t2b.ptr, n1b.ptr,
                                          n2b.ptr, n3b.ptr, badb.ptr, errb.ptr, bounds.ptr if frame_rows else None,
                                          WIRE_FRAME_ROWS if frame_rows else 0, stream))
    else:
        check(lib.pekf_wire_events_ext_dev(K, F, fb.ptr, F, F, ev2.ptr, ev3.ptr, t2b.ptr, n2b.ptr, n3b.ptr, badb.ptr,
                                           errb.ptr, bounds.ptr if frame_rows else None,
                                           WIRE_FRAME_ROWS if frame_rows else 0, stream))
    check(lib.pekf_device_sync() if stream is None else lib.pekf_stream_sync(stream))
    n2, n3 = n2b.download((K,), np.int32), n3b.download((K,), np.int32)
    dead = None if stopped is None or not np.any(stopped) else np.asarray(stopped, bool).reshape(K)
    bad = None
    if int(errb.download((1,), np.int32)[0]) & 1:
        bad = badb.download((K,), np.int32)
        if dead is not None:   # (a phone whose stream has ended sends nothing that counts)
            bad = np.where(dead, -1, bad).astype(np.int32)
        if refused == "raise" and (bad >= 0).any():
            k = int(np.argmax(bad >= 0))
            raise ValueError("phone %d, frame %d: not in the client's message form (wire.parse reads it)" % (k, bad[k]))
    n1 = n1b.download((K,), np.int32) if phase1 else None
    if frame_rows:  # the rows that hold messages of any phone: ev2's first E2, ev3's from row F - E3, ev1's first E1
        bw = bounds.download((3 if phase1 else 2,), np.int32)
        E2, E3, E1 = int(bw[0]), int(bw[1]), int(bw[2]) if phase1 else 0
    else:
        E2, E3 = int(n2.max(initial=0)), int(n3.max(initial=0))
        E1 = int(n1.max(initial=0)) if phase1 else 0
    out = dict(ev2=ev2, ev3=ev3, E2=E2, E3=E3, ev3_from=F - E3 if frame_rows else 0, n2=n2, n3=n3,
               first_t2=t2b, frames=fb)
    if phase1:
        out.update(ev1=ev1, E1=E1, n1=n1)
    bad_frame, repaired = np.full(K, -1, np.int32), np.zeros(K, bool)
    if F and (dead is not None or (bad is not None and (bad >= 0).any())):   # (refused == "raise": dead columns only)
        bad_frame, repaired = _repair_wire(out, (n1b if phase1 else None, n2b, n3b, badb), frames, F, K, stream,
                                           frame_rows, phase1, np.full(K, -1, np.int32) if bad is None else bad,
                                           bounds, dead)
    if refused == "repair":
        out.update(bad_frame=bad_frame, repaired=repaired)
    return out


def run_wire_session(frames, filters, n_avg=100, alpha=0.1, stream=None, frame_rows=True, calibration=None,
                     n_cal=100, trajectory=False, refused="raise"):
    """A whole client session from the clients' wire frames, on the device end to end (KFS/Server.cpp's
    recv'd frames -> Parser.cpp:28-72): pekf_wire_events_ext_dev (the server's parse into FP64 event
    planes), pekf_frontend_init_ext_dev (phase 2) and pekf_live_ext_dev (phase 3 + the filter) on the
    server's own values, no host parse.  filters: a BatchedEKF (FP64, AoS).  Returns run_session's dict,
    the same with or without frame_rows.  frame_rows (default): planes with a row per frame index (see
    wire_events), whose stores stay coalesced when the phones' phase-1 / phase-2 parts differ in length
    and whose frames a small batch splits over several waves; phase 2 and phase 3 read only the rows that
    hold messages (65,536 phones: 5.0 ms against 6.0 compacted with aligned rows, 5.0 against 8.0 ms with
    rows 64 apart).  calibration: as run_session (a dict: calibrate_magnetometer's, made elsewhere), or
    "frames": phase 1 from the same frames, on the device and on the session's stream -- the parse keeps the
    phase-1 messages (pekf_wire_events_p1_dev), pekf_magcal_dev fits each phone's first n_cal of them wherever
    they sit in its stream, and pekf_magcal_apply_dev corrects the whole of phases 2 and 3; the returned dict
    then also has calibration, the dict calibrate_magnetometer returns.  The only host round trip is
    wire_events' own (the error word and the bounds).  trajectory: as run_session (True: a row per three of
    the phase-3 rows the launch reads), from the same launch, with either kind of rows and any calibration.
    refused: as wire_events.  "raise" (default): a frame the device parser does not take raises ValueError, for the
    whole batch.  "repair": only its phone is affected -- the host reads that phone's frames from it on and the
    session goes on (with no refused frame the launches are the same); the dict gains bad_frame (K,) int32 and
    repaired (K,) bool, wire_events'.  A stopped phone (bad_frame >= 0: a frame the server's std::stod / std::stoll
    throw on, which ends that client's server process) is a phone whose stream ended at that frame: it keeps
    whatever ready, counts and state it had reached.
    Raises ValueError, before anything is launched, if
    filters.batch is not the frames' phone count, calibration is another string or refused an unknown one."""
    K = filters.batch
    _check_refused(refused)
    _scalar_noise_only(filters, "run_wire_session", "PhoneSession (feed_frames)")
    from_frames = isinstance(calibration, str)
    if from_frames and calibration != "frames":
        raise ValueError("calibration must be None, calibrate_magnetometer's dict or 'frames'")
    Kf = _frames_shape(frames)[1]
    if Kf != K:  # the planes' column stride is the frames' phone count: any other batch reads them wrong
        raise ValueError("the frames are of %d phones, the filters of %d" % (Kf, K))
    w = wire_events(frames, stream, frame_rows, phase1=from_frames, refused=refused)
    if from_frames:
        calibration = _launch_calibration(K, w["E1"], w["ev1"].ptr, n_cal, EV_F64_EVENTS, stream)
    if calibration is not None:  # with frame rows the no-message rows are walked too (and left as they are)
        _apply_calibration(calibration, K, w["E2"], w["ev2"].ptr, EV_F64_EVENTS, stream)
        _apply_calibration(calibration, K, w["E3"], w["ev3"].ptr + 32 * K * w["ev3_from"], EV_F64_EVENTS, stream)
    p2 = _launch_phase2(K, w["E2"], w["ev2"].ptr, w["first_t2"], n_avg, EV_F64_EVENTS, stream)
    ev3 = w["ev3"]
    if w["ev3_from"]:  # (frame rows) the leading rows no phone has a phase-3 message in
        ev3 = types.SimpleNamespace(ptr=ev3.ptr + 32 * K * w["ev3_from"])
    out = _finish_session(filters, ev3, w["E3"], p2, alpha, EV_F64_EVENTS, trajectory, calibration, stream,
                          from_frames)
    if refused == "repair":
        out.update(bad_frame=w["bad_frame"], repaired=w["repaired"])
    return out


# ------------------------------------------------------------------ the batched filter

def _run_flags(precision, layout):
    """the PEKF_RUN_* flags of a filter's precision and state layout"""
    return (RUN_MIXED_PRECISION if precision == "mixed" else 0) | (RUN_STATE_SOA if layout == "soa" else 0)


def _launch_counts(win, counts, n_steps, step0):
    """A run's per-filter record counts as a DeviceBuffer of batch int32 (or None: every filter runs n_steps).
    counts: an array of batch ints or a DeviceBuffer; default win.counts (ragged logs / front-end output) shifted
    by step0, so each filter applies exactly its own records while sharing one launch."""
    if counts is None and win.counts is not None:
        counts = np.clip(np.asarray(win.counts, np.int64) - int(step0), 0, n_steps)
    if counts is None or isinstance(counts, DeviceBuffer):
        return counts
    c = np.ascontiguousarray(counts, dtype=np.int32).reshape(win.batch)
    return DeviceBuffer(c.nbytes).upload(c)


def _noise_arrays(q, r, n, what="batch"):
    """q and r, each a scalar or an array-like of n values, as two (n,) float64 arrays; refuses, on the host, a
    wrong shape, a non-finite value, r <= 0 and q < 0 (the device entries' precondition, include/pekf.h)."""
    out = []
    for name, v in (("q", q), ("r", r)):
        a = np.asarray(v, dtype=np.float64)
        if a.ndim > 1 or (a.ndim == 1 and a.shape != (n,)):
            raise ValueError("%s must be a scalar or %d values (one per %s), not of shape %s" % (name, n, what, a.shape))
        a = np.array(np.broadcast_to(a, (n,)))   # (a copy: the filter's own arrays)
        if not np.isfinite(a).all():
            raise ValueError("every %s must be finite" % name)
        out.append(a)
    if (out[1] <= 0).any():
        raise ValueError("every r must be > 0 (S = P- + rI must be SPD)")
    if (out[0] < 0).any():
        raise ValueError("every q must be >= 0")
    return out[0], out[1]


class BatchedEKF:
    """B independent filters of the reference model, state resident on the device.

    Equivalent, filter by filter, to the reference's main_file.py:19-47 driver:
    KalmanFilter(T0, mag_0, acc_0) with setQ(q), setR(r), P = I, X = [1,0,0,0], then
    Prediction + Correction for every record.  `run` advances all filters n_steps records.

    Noise, launch-wide or per filter.  Two scalars q and r: one Q = qI and R = rI for the whole batch, kernel
    arguments of every launch (self.noise is None).  If either is an array-like of `batch` values, the filter has
    per-filter noise: self.q and self.r are (batch,) float64 arrays and self.noise is a DeviceBuffer of 16 B per
    filter, {q, r}, which run / run_async (all three window kinds), LiveSession and PhoneSession hand to the
    per-filter-noise kernels (pekf_*_noise_dev); a filter whose pair is (q, r) gets the scalar launch's bits.
    self.noise is written by the constructor, by set_noise -- for the run paths, where P is stored plain between
    launches -- and by PhoneSession.recycle(q=, r=).  Recycling is the only point at which a live session
    column's noise may change: the session state holds the covariance in an r-scaled form (N, with P = rI +
    sqrt(2) r D N D), so changing a column's r in mid-session would reinterpret its P.
    Scalar-only: FilterHandle, the drop-ins, the one-record online path (a per-filter launch of one record runs
    the multi-record arithmetic), the side-output kernels, precision="mixed", layout="soa" and
    shard.MultiDeviceEKF.
    """

    def __init__(self, batch, q=1.0, r=0.1, precision="f64", layout="aos"):
        """precision: "f64" (default, as the reference) or "mixed" (covariance path in f32).
        layout: "aos" (X[B][4], P[B][4][4]) or "soa" (X[4][B], P[10][B]: coalesced state access,
        for launches that cover few records, e.g. online serving).
        q, r: each a scalar or an array-like of batch values (per-filter noise: FP64 on AoS state only)."""
        if precision not in ("f64", "mixed"):
            raise ValueError("precision must be 'f64' or 'mixed'")
        if layout not in ("aos", "soa"):
            raise ValueError("layout must be 'aos' or 'soa'")
        self.batch = int(batch)
        self.noise = None
        if np.ndim(q) == 0 and np.ndim(r) == 0:
            self.q, self.r = float(q), float(r)
        else:   # validated on the host, before any device call
            if precision != "f64" or layout != "aos":
                raise ValueError("per-filter noise (array q / r) runs the FP64 filter on AoS state: not with "
                                 "precision='mixed' or layout='soa'")
            self.q, self.r = _noise_arrays(q, r, self.batch)
            self.noise = DeviceBuffer(16 * self.batch).upload(np.stack([self.q, self.r], axis=1))
        self.layout = layout
        self.flags = _run_flags(precision, layout)
        self.X = DeviceBuffer(32 * self.batch)
        self.P = DeviceBuffer((80 if layout == "soa" else 128) * self.batch)
        self.reset()

    @property
    def per_filter_noise(self):
        """True if q and r are per filter (self.noise holds them on the device)"""
        return self.noise is not None

    def same_noise(self, q, r):
        """True if this filter's q and r equal the given ones (scalars or arrays), as restore needs them"""
        return (np.ndim(q) == np.ndim(self.q) and np.ndim(r) == np.ndim(self.r) and
                np.array_equal(self.q, q) and np.array_equal(self.r, r))

    def set_noise(self, columns, q, r):
        """New noise for the listed columns of a per-filter-noise filter: q and r scalars or one value per listed
        column, validated as the constructor's, written to self.q / self.r and to those entries of self.noise
        (synchronous).  For the run paths, where P is stored plain between launches; a live session's column may
        change its noise only when it is recycled (PhoneSession.recycle(q=, r=), which calls this)."""
        if self.noise is None:
            raise ValueError("set_noise needs a per-filter-noise filter: construct BatchedEKF with array q / r")
        cols = _recycle_columns(columns, self.batch)
        qn, rn = _noise_arrays(q, r, len(cols), "listed column")
        if len(cols) == 0:
            return
        self.q[cols], self.r[cols] = qn, rn
        lo, hi = int(cols.min()), int(cols.max()) + 1   # one copy of the range that holds them
        part = np.ascontiguousarray(np.stack([self.q[lo:hi], self.r[lo:hi]], axis=1))
        check(lib.pekf_memcpy_h2d(self.noise.ptr + 16 * lo, part.ctypes.data, part.nbytes, None))
        check(lib.pekf_device_sync())

    def _to_layout(self, Xa, Pa, to_soa, stream=None):
        check(lib.pekf_state_layout_dev(self.batch, Xa.ptr, Pa.ptr, self.X.ptr, self.P.ptr, int(to_soa), stream))

    def reset(self, stream=None):
        if self.layout == "soa":
            Xa, Pa = DeviceBuffer(32 * self.batch), DeviceBuffer(128 * self.batch)
            check(lib.pekf_reset_state_dev(self.batch, Xa.ptr, Pa.ptr, stream))
            self._to_layout(Xa, Pa, True, stream)
        else:
            check(lib.pekf_reset_state_dev(self.batch, self.X.ptr, self.P.ptr, stream))
        check(lib.pekf_device_sync() if stream is None else lib.pekf_stream_sync(stream))

    def set_state(self, X, P):
        """X (B, 4), P (B, 4, 4) in the reference's row-major layout, whatever self.layout is."""
        X, P = f64(X, (self.batch, 4)), f64(P, (self.batch, 4, 4))
        if self.layout == "soa":
            Xa, Pa = DeviceBuffer(X.nbytes).upload(X), DeviceBuffer(P.nbytes).upload(P)
            self._to_layout(Xa, Pa, True)
            check(lib.pekf_device_sync())
        else:
            self.X.upload(X)
            self.P.upload(P)

    def get_state(self):
        """(X (B, 4), P (B, 4, 4)) in the reference's row-major layout."""
        if self.layout == "soa":
            Xa, Pa = DeviceBuffer(32 * self.batch), DeviceBuffer(128 * self.batch)
            self._to_layout(Xa, Pa, False)
            check(lib.pekf_device_sync())
            return Xa.download((self.batch, 4), np.float64), Pa.download((self.batch, 4, 4), np.float64)
        return (self.X.download((self.batch, 4), np.float64),
                self.P.download((self.batch, 4, 4), np.float64))

    def run_async(self, win: IMUWindow, n_steps, step0=0, stream=None, traj=None, counts=None):
        """Enqueue one fused launch; traj: optional DeviceBuffer of n_steps*batch*32 bytes;
        counts: optional DeviceBuffer of batch int32 (filter b applies its first counts[b] records).
        A window with a dt side plane (escaped records) runs pekf_run_ext_dev with it; a RecordWindow64
        (FP64 records) runs pekf_run_rec64_dev.  A per-filter-noise filter runs their pekf_run_noise_dev /
        pekf_run_rec64_noise_dev (always the multi-record arithmetic, also for one record)."""
        assert win.batch == self.batch
        tr, cn = traj.ptr if traj is not None else None, counts.ptr if counts is not None else None
        if self.noise is not None:
            if isinstance(win, RecordWindow64):
                check(lib.pekf_run_rec64_noise_dev(self.batch, int(n_steps), win.window, int(step0), win.gd.ptr,
                                                   win.am.ptr, win.my.ptr, win.refs.ptr, self.X.ptr, self.P.ptr,
                                                   self.noise.ptr, tr, cn, stream))
            else:
                check(lib.pekf_run_noise_dev(self.batch, int(n_steps), win.window, int(step0), win.gd.ptr, win.am.ptr,
                                             win.my.ptr, win.dtx.ptr if win.dtx is not None else None, win.refs.ptr,
                                             self.X.ptr, self.P.ptr, self.noise.ptr, tr, cn, self.flags, stream))
        elif isinstance(win, RecordWindow64):
            if self.layout != "aos" or self.flags & RUN_MIXED_PRECISION:
                raise ValueError("FP64-record windows run the FP64 filter on AoS state")
            check(lib.pekf_run_rec64_dev(self.batch, int(n_steps), win.window, int(step0), win.gd.ptr, win.am.ptr,
                                         win.my.ptr, win.refs.ptr, self.X.ptr, self.P.ptr, self.q, self.r, tr, cn,
                                         stream))
        elif win.dtx is None:
            check(lib.pekf_run_dev(self.batch, int(n_steps), win.window, int(step0), win.gd.ptr, win.am.ptr,
                                   win.my.ptr, win.refs.ptr, self.X.ptr, self.P.ptr, self.q, self.r, tr, cn,
                                   self.flags, stream))
        else:
            check(lib.pekf_run_ext_dev(self.batch, int(n_steps), win.window, int(step0), win.gd.ptr, win.am.ptr,
                                       win.my.ptr, win.dtx.ptr, win.refs.ptr, self.X.ptr, self.P.ptr, self.q,
                                       self.r, tr, cn, self.flags, stream))

    def run(self, win: IMUWindow, n_steps=None, step0=0, want_traj=False, counts=None):
        """Advance every filter n_steps records (default: the whole window) from row step0.

        counts: per-filter record counts for this launch (_launch_counts: default win.counts from step0 on)."""
        n_steps = win.window if n_steps is None else int(n_steps)
        tb = DeviceBuffer(32 * n_steps * self.batch) if want_traj else None
        self.run_async(win, n_steps, step0, None, tb, _launch_counts(win, counts, n_steps, step0))
        check(lib.pekf_device_sync())
        if want_traj:
            return tb.download((n_steps, self.batch, 4), np.float64)
        return None

    def run_events_async(self, ev_planes, n_events, init, t_init, counts, refs, alpha=0.1, stream=None, flags=0,
                         traj=None, traj_dt=None, traj_rows=0):
        """Enqueue pekf_live_ext_dev: device event planes [n_events][batch][4] f32 (synth.pack_events), init
        (batch, 6), t_init (batch,) int64; counts (batch,) int32 and refs (batch, 6) outputs -- DeviceBuffers;
        flags: EV_TIME_EVENTS if the planes hold time events, EV_F32_RECORDS for f32 records.
        traj_rows > 0: pekf_live_traj_dev instead, each filter's X after its r-th record (r < traj_rows) into
        traj, a DeviceBuffer [traj_rows][batch][4] float64, and its dt in ns into traj_dt [traj_rows][batch]
        (optional); rows a filter does not reach are not written."""
        if self.layout != "aos" or self.flags & RUN_MIXED_PRECISION:
            raise ValueError("the fused front-end + filter kernel runs the FP64 filter on AoS state")
        if self.noise is not None:   # (never silently with a scalar)
            raise ValueError("the one-launch live kernels take one q and one r: feed a per-filter-noise filter "
                             "through LiveSession (phase-3 events) or PhoneSession (a session from its first "
                             "message, wire frames included) instead")
        traj_rows = int(traj_rows)
        if traj_rows < 0:
            raise ValueError("traj_rows must be >= 0")
        if traj_rows == 0:
            check(lib.pekf_live_ext_dev(self.batch, int(n_events), ev_planes.ptr, init.ptr, t_init.ptr, float(alpha),
                                        self.X.ptr, self.P.ptr, self.q, self.r, counts.ptr, refs.ptr, int(flags), None,
                                        stream))
            return
        if traj is None or traj.nbytes < 32 * traj_rows * self.batch:
            raise ValueError("traj must be a DeviceBuffer of traj_rows * batch * 32 bytes")
        if traj_dt is not None and traj_dt.nbytes < 8 * traj_rows * self.batch:
            raise ValueError("traj_dt must be a DeviceBuffer of traj_rows * batch * 8 bytes")
        check(lib.pekf_live_traj_dev(self.batch, int(n_events), ev_planes.ptr, init.ptr, t_init.ptr, float(alpha),
                                     self.X.ptr, self.P.ptr, self.q, self.r, counts.ptr, refs.ptr, int(flags),
                                     traj.ptr, traj_dt.ptr if traj_dt is not None else None, traj_rows, None, stream))

    def run_events(self, ev, alpha=0.1, records="f64", events="f32", trajectory=False):
        """Raw phone events (synth.generate_events layout) -> front-end -> filter, fused in one launch
        (pekf_live_ext_dev).  Returns (counts (batch,) int32 records applied, refs (batch, 6)
        the filters' acc0 / mag0).  Any event gap and any record dt is applied (time events, escapes).
        records: "f64" (default) feeds the filter the FP64 low-pass acc / mag, as the server does
        (KFS/KalmanFilter.cpp:279-303); "f32" rounds them to the 40 B stream record first, which makes the
        result equal run_frontend + run bit for bit.
        events: "f32" the float32 samples (16 B events); "f64" the server's own values (32 B events,
        server_event_values: what std::stod parses from the phone's text), every record field FP64 --
        equal to run_frontend(events="f64") + run bit for bit.
        trajectory: True or a row cap (True: n_events // 3) adds a third value, run_session's dict of
        trajectory (R, batch, 4), record_dt_ns (R, batch) and record_times_ns (R, batch): a pose per record,
        from the same launch."""
        assert np.asarray(ev["types"]).shape[1] == self.batch
        _scalar_noise_only(self, "run_events", "LiveSession")
        evb, E, flags = _event_planes(ev, events)
        init = DeviceBuffer(48 * self.batch).upload(
            np.concatenate([ev["init_acc"], ev["init_mag"]], axis=1).astype(np.float64))
        tib = DeviceBuffer(8 * self.batch).upload(np.ascontiguousarray(ev["t_init"], np.int64))
        cnt, refs, tj = _run_live(self, evb, E, init, tib, alpha, flags | _record_flags(records, events), trajectory)
        out = cnt.download((self.batch,), np.int32), refs.download((self.batch, 6), np.float64)
        return out + (tj.result(ev["t_init"]),) if tj.wanted else out


def chunk_trajectory_rows(trajectory, n_events):
    """trajectory_rows for one chunk of a LiveSession: True is (n_events + 2) // 3 rows, since a chunk's first
    record may need one event only (its gyro and the other sample came in earlier chunks), every later one three."""
    return (int(n_events) + 2) // 3 if trajectory is True else trajectory_rows(trajectory, n_events)


def _recycle_columns(columns, batch):
    """recycle's `columns` as (n,) int32 in the caller's order; refuses what is not a 1-D list of distinct
    integer indices in [0, batch)"""
    cols = np.asarray(columns)
    if cols.size == 0 and cols.ndim == 1:
        return np.zeros(0, np.int32)
    if cols.ndim != 1 or not np.issubdtype(cols.dtype, np.integer):
        raise ValueError("columns must be a 1-D sequence of integer column indices")
    if cols.min() < 0 or cols.max() >= batch:
        raise ValueError("columns must lie in [0, %d)" % batch)
    if len(np.unique(cols)) != len(cols):
        raise ValueError("columns lists a column twice")
    return np.ascontiguousarray(cols, np.int32)


def _launch_recycle(batch, cols, filter_group=None, phase2_group=None, phase1_group=None):
    """pekf_session_recycle_dev on the host list cols, run to completion.  The groups are the entry's, as tuples
    in its argument order with None for what is not given: (state, X, P, refs, X0, P0, final_X, final_P),
    (state, t_start, init, t_init, ready, t_start_new), (state, n_cal, cal, fit, status)."""
    dev = DeviceBuffer(4 * len(cols)).upload(cols)
    f, p2, p1 = filter_group or (None,) * 8, phase2_group or (None,) * 6, phase1_group or (None, 0, None, None, None)
    check(lib.pekf_session_recycle_dev(batch, len(cols), dev.ptr, EV_F64_EVENTS if filter_group else 0, *f, *p2, *p1,
                                       None))
    check(lib.pekf_device_sync())


def _launch_move(entry, batch, cols, flags, pack, filter_group=None, phase2_group=None, phase1_group=None):
    """pekf_session_export_dev / pekf_session_import_dev (entry) on the host list cols and the DeviceBuffer pack,
    run to completion.  The groups are the entries', as tuples in their argument order: (state, X, P, refs),
    (state, t_start, init, t_init, ready), (state, n_cal, cal, fit, status)."""
    dev = DeviceBuffer(4 * len(cols)).upload(cols)
    f, p2, p1 = filter_group or (None,) * 4, phase2_group or (None,) * 5, phase1_group or (None, 0, None, None, None)
    check(entry(batch, len(cols), dev.ptr, flags, *f, *p2, *p1, pack.ptr, None))
    check(lib.pekf_device_sync())


class SessionColumns:
    """Live phones out of their session (PhoneSession.export_columns, CalibrationSession.export_columns): the
    columns' device state in one packed DeviceBuffer (pekf_session_export_dev; its layout is private) and what
    the host holds for them.  import_columns of a session with the same n_avg, alpha and n_cal takes them, in
    this object's order; to_host / from_host carry them to another process or device.

    kind: "phone" (a PhoneSession's columns: the filter, phase 2 and, with n_cal, phase 1) or "calibration" (a
    CalibrationSession's: phase 1 alone); n: the columns; n_avg, alpha (a phone's), n_cal (None: no phase 1),
    events; q, r (n,): the columns' noise -- the session state holds the covariance scaled by r, so they travel
    with it; book: the columns' rows of the session's host book, dict of (n,) arrays (a phone's t_init, dt_sum,
    total_counts; an f32 calibration's last_times)."""

    def __init__(self, kind, pack, n, n_avg, alpha, n_cal, events, q, r, book):
        self.kind, self.pack, self.n = kind, pack, int(n)
        self.n_avg, self.alpha, self.n_cal, self.events = n_avg, alpha, n_cal, events
        self.q, self.r, self.book = q, r, book

    @property
    def flags(self):
        """the pack's flags (pekf_session_columns_bytes): a phone's pack is a joining session's"""
        return EV_F64_EVENTS if self.kind == "phone" else 0

    @staticmethod
    def nbytes(n, n_cal, flags):
        nbytes = int(lib.pekf_session_columns_bytes(n, n_cal or 0, flags))
        if nbytes < 0:
            raise ValueError("no pack for %d columns with n_cal=%r" % (n, n_cal))
        return nbytes

    def to_host(self):
        """The object as a dict of NumPy arrays (the pack's bytes as uint8; scalars as 0-d arrays, -1 for a
        missing n_avg / n_cal and NaN for a missing alpha); from_host rebuilds it."""
        d = dict(kind=np.array(self.kind), events=np.array(self.events), n=np.array(self.n, np.int64),
                 n_avg=np.array(-1 if self.n_avg is None else self.n_avg, np.int64),
                 n_cal=np.array(-1 if self.n_cal is None else self.n_cal, np.int64),
                 alpha=np.array(np.nan if self.alpha is None else self.alpha, np.float64),
                 q=self.q.copy(), r=self.r.copy(), pack=self.pack.download((self.pack.nbytes,), np.uint8))
        d.update(("book_" + name, rows.copy()) for name, rows in self.book.items())
        return d

    @classmethod
    def from_host(cls, d):
        """to_host's dict as an object on the current device (set_device first to move a phone to another one)"""
        kind, n = str(d["kind"]), int(d["n"])
        if kind not in ("phone", "calibration"):
            raise ValueError("kind must be 'phone' or 'calibration'")
        n_avg, n_cal = (None if int(d[key]) < 0 else int(d[key]) for key in ("n_avg", "n_cal"))
        alpha = None if np.isnan(d["alpha"]) else float(d["alpha"])
        book = {key[5:]: np.array(rows) for key, rows in d.items() if key.startswith("book_")}
        q, r = np.array(d["q"], np.float64), np.array(d["r"], np.float64)
        pack = np.ascontiguousarray(d["pack"], np.uint8)
        if any(np.shape(a) != (n,) for a in (q, r) + tuple(book.values())):
            raise ValueError("q, r and the book rows must have one entry per column")
        if pack.shape != (cls.nbytes(n, n_cal, EV_F64_EVENTS if kind == "phone" else 0),):
            raise ValueError("the pack's bytes are not those of %d columns with n_cal=%r" % (n, n_cal))
        buf = DeviceBuffer(pack.nbytes)
        if pack.nbytes:
            buf.upload(pack)
        return cls(kind, buf, n, n_avg, alpha, n_cal, str(d["events"]), q, r, book)


def _import_refusals(session, kind, cols, pack, fields):
    """import_columns' refusals that do not depend on the session's class, before any launch"""
    if not isinstance(pack, SessionColumns) or pack.kind != kind:
        raise ValueError("import_columns takes the SessionColumns of a session of this class (export_columns)")
    if len(cols) != pack.n:
        raise ValueError("%d columns listed for a pack of %d" % (len(cols), pack.n))
    for name in fields:
        if getattr(session, name) != getattr(pack, name):
            raise ValueError("the pack's %s is %r, the session's %r: a phone moves between sessions of the same "
                             "n_avg, alpha and n_cal" % (name, getattr(pack, name), getattr(session, name)))


class _ChunkedSession:
    """A session fed in chunks, what LiveSession and PhoneSession share: the filters it refuses, the host
    bookkeeping (the summed counts, the running record times), what follows a chunk's launch, and snapshot /
    restore.  A subclass allocates its DeviceBuffers as self._<name> (_cnt and _refs among them), launches, and
    states three things: _BUFFERS, the buffers a snapshot carries (name -> None: its bytes as uint8, or n: (K, n)
    float64); _FIELDS, the constructor's scalars it carries; _from_snapshot, the empty session restore fills."""

    _BUFFERS, _FIELDS = {}, ()

    def __init__(self, filters):
        if filters.layout != "aos" or filters.flags & RUN_MIXED_PRECISION:
            raise ValueError("the fused front-end + filter kernel runs the FP64 filter on AoS state")
        K = filters.batch
        self.filters, self.batch = filters, K
        self._book = dict(started=False, t_init=np.zeros(K, np.int64), dt_sum=np.zeros(K),
                          total_counts=np.zeros(K, np.int64))

    @property
    def total_counts(self):
        """(K,) int64: the records each filter has applied since the session began"""
        return self._book["total_counts"].copy()

    @property
    def refs(self):
        """(K, 6) the filters' acc0 / mag0 as of the last chunk (written by every launch; before the first, from
        a zero-row one; NaN for a phone that is not ready)"""
        if not self._book["started"]:
            self._feed_no_rows()
        return self._refs.download((self.batch, 6), np.float64)

    @staticmethod
    def _rows_in(planes, n, offset, row_bytes):
        """Refuses n rows of row_bytes, `offset` bytes into the DeviceBuffer planes, that are not all inside it"""
        if n < 0 or offset < 0 or offset % 16 or (n > 0 and (planes is None or offset + n * row_bytes > planes.nbytes)):
            raise ValueError("offset / rows outside the planes buffer (or offset not a multiple of 16)")

    def _after_launch(self, tj):
        """What follows a chunk's launches: the sync, the chunk's counts, the bookkeeping.  Returns (counts,), or
        with a trajectory asked for (tj: the launch's _Trajectory) (counts, its dict)."""
        K, book = self.batch, self._book
        check(lib.pekf_device_sync())
        book["started"] = True
        counts = self._cnt.download((K,), np.int32)
        self._first_records((book["total_counts"] == 0) & (counts > 0))
        book["total_counts"] += counts
        if not tj.wanted:
            book["dt_sum"] = np.where(counts > 0, np.nan, book["dt_sum"])   # these records' dts were not asked for
            return (counts,)
        return counts, self._chunk_result(tj.result(np.zeros(K)), counts)

    def _first_records(self, first):
        """first (K,) bool: the filters whose first record of the session was applied in this chunk"""

    @staticmethod
    def _records_trajectory(trajectory, records):
        """records=True implies a trajectory: without one asked for, the chunk's default row cap (True)"""
        return True if records and (trajectory is None or trajectory is False) else trajectory

    def _noise_args(self):
        """(q, r, noise) of a _rec entry: the launch's q and r with a NULL plane, or the filter's {q, r} plane"""
        f = self.filters
        return (f.q, f.r, None) if f.noise is None else (0.0, 0.0, f.noise.ptr)

    def _with_records(self, out, win):
        """Adds "records" to a chunk's trajectory dict: the chunk's RecordWindow64 (_chunk_records, filled by the
        launch) with the session's refs and counts = min(the chunk's counts, its rows) -- device-resident, as
        BatchedEKF.run, gyro_chain, wahba_quaternions and download_filters take it.  win.chunk_counts: the chunk's
        full counts (a filter whose count is above the window's rows had records cut by the row cap)."""
        counts = out[0]
        check(lib.pekf_memcpy_d2d(win.refs.ptr, self._refs.ptr, 48 * self.batch, None))
        check(lib.pekf_device_sync())
        win.counts = np.minimum(counts, win.window).astype(np.int32)
        win.chunk_counts = np.array(counts, np.int32)
        out[-1]["records"] = win
        return out

    def _chunk_result(self, out, counts):
        """The chunk's trajectory dict with record_times_ns continuing from the session's running record time: per
        filter t_init + the running sum of every dt so far, summed in the order one launch's cumsum would.  A
        filter whose earlier records' dts were not all downloaded (a chunk fed without a trajectory, or with a
        row cap below its count) has NaN times from then on."""
        book, dt = self._book, out["record_dt_ns"]
        run = np.cumsum(np.concatenate([book["dt_sum"][None, :], dt], axis=0), axis=0)
        out["record_times_ns"] = book["t_init"].astype(np.float64)[None, :] + run[1:]
        seen = np.minimum(counts, len(dt))
        last = run[seen, np.arange(self.batch)]
        book["dt_sum"] = np.where(counts > len(dt), np.nan, last)
        return out

    def snapshot(self):
        """The session as host data: dict(batch, q, r (arrays for a per-filter-noise filter), the class's scalars, its device buffers -- the session
        state(s) as bytes (uint8 arrays) -- X, P and the host-side bookkeeping).  restore continues from it on
        another BatchedEKF or device."""
        K = self.batch
        X, P = self.filters.get_state()
        snap = dict(batch=K, q=copy.copy(self.filters.q), r=copy.copy(self.filters.r), X=X, P=P,
                    book=copy.deepcopy(self._book))
        snap.update((name, getattr(self, name)) for name in self._FIELDS)
        for name, cols in self._BUFFERS.items():
            buf = getattr(self, "_" + name)
            snap[name] = buf.download((buf.nbytes,), np.uint8) if cols is None else buf.download((K, cols), np.float64)
        return snap

    @classmethod
    def restore(cls, filters, snapshot):
        """A session that continues `snapshot` on `filters` (same batch, q and r -- for per-filter noise the same
        arrays, compared with np.array_equal; set the device first to move a shard): its X / P are set to the snapshot's, the buffers are uploaded as they were."""
        s = snapshot
        if filters.batch != s["batch"] or not filters.same_noise(s["q"], s["r"]):
            raise ValueError("restore needs a BatchedEKF of the snapshot's batch, q and r")
        self = cls._from_snapshot(filters, s)
        filters.set_state(s["X"], s["P"])
        for name in self._BUFFERS:
            getattr(self, "_" + name).upload(s[name])
        self._book = copy.deepcopy(s["book"])
        return self


class LiveSession(_ChunkedSession):
    """A live session fed in chunks (pekf_live_resume_dev): the phones' phase-3 events as they arrive, a launch
    per chunk, the front-end's and the filter's state carried between them on the device.  However the events are
    cut into chunks, X, P, refs, the summed counts and the concatenated trajectory rows have the bits of
    BatchedEKF.run_events on all of them at once.

    filters: a BatchedEKF (FP64, AoS) -- its X / P start the session and receive, after every chunk, the X_k / P of
    the filters that applied a record in it; while the session runs they are outputs only (the session state
    holds the filter).  init_acc / init_mag (K, 3) host arrays of the raw phase-2 means, or init_acc a DeviceBuffer
    of phase 2's init (K, 6) and init_mag None (_launch_phase2's); t_init (K,) int64 host array or DeviceBuffer.
    events: "f32" or "f64", fixed for the session (records are FP64 either way).

    Its columns cannot be recycled (PhoneSession.recycle): every lane starts from the launch's one `resume` word,
    so there is no per-lane fresh start; that needs the joining kernels on f32 events."""

    _BUFFERS, _FIELDS = dict(state=None, init=6, refs=6), ("events", "alpha")

    def __init__(self, filters, init_acc, init_mag, t_init, alpha=0.1, events="f32"):
        if events not in EVENT_FORMS:
            raise ValueError("events must be 'f32' or 'f64'")
        super().__init__(filters)
        K = self.batch
        self.alpha, self.events = float(alpha), events
        self._form = EV_F64_EVENTS if events == "f64" else 0
        if isinstance(init_acc, DeviceBuffer):
            self._init = init_acc
        else:
            init = np.concatenate([np.asarray(init_acc, np.float64).reshape(K, 3),
                                   np.asarray(init_mag, np.float64).reshape(K, 3)], axis=1)
            self._init = DeviceBuffer(48 * K).upload(init)
        if isinstance(t_init, DeviceBuffer):
            self._t_init, t_host = t_init, t_init.download((K,), np.int64)
        else:
            t_host = np.ascontiguousarray(t_init, np.int64).reshape(K).copy()
            self._t_init = DeviceBuffer(8 * K).upload(t_host)
        nbytes = int(lib.pekf_live_state_bytes(K, self._form))
        if nbytes < 0:
            raise ValueError("no session state for these flags")
        self._state, self._cnt, self._refs = DeviceBuffer(nbytes), DeviceBuffer(4 * K), DeviceBuffer(48 * K)
        self._book.update(t_init=t_host, last_times=t_host.copy())

    @classmethod
    def _from_snapshot(cls, filters, s):   # (init: an empty buffer, uploaded with the others)
        return cls(filters, DeviceBuffer(48 * s["batch"]), None, s["book"]["t_init"], s["alpha"], s["events"])

    def _feed_no_rows(self):
        self.feed_planes(self._state, 0)   # (no rows: any valid pointer, none is read)

    def pack_chunk(self, ev):
        """A chunk's rows (types / values / times, optionally values64) -> (host planes, PEKF_EV_* flags) in the
        session's event form.  f32: synth.pack_events with the chunk's first gap taken from the previous chunk's
        last times row (t_init before the first), which the session keeps; null padding lands mid-stream."""
        times = np.asarray(ev["times"], np.int64)
        chunk = dict(ev, t_init=self._book["last_times"])
        if self.events == "f64":
            planes, flags = synth.pack_events64(chunk, server_event_values(chunk)), EV_F64_EVENTS
        else:
            planes = synth.pack_events(chunk)
            flags = EV_TIME_EVENTS if synth.has_time_events(planes) else 0
        if len(times):
            self._book["last_times"] = times[-1].copy()
        return planes, flags

    def feed(self, ev, trajectory=False, records=False):
        """The next rows of every filter's stream: a synth.generate_events-style dict of types (E, K), values
        (E, K, 3), times (E, K) and optionally values64 (init_* / t_init entries are ignored).  Returns counts
        (K,) int32, the records applied in this chunk, or with trajectory (True or a row cap) (counts, dict of
        trajectory / record_dt_ns / record_times_ns) as run_events does, rows counted within the chunk.
        records=True (pekf_live_resume_rec_dev; it implies trajectory=True where none is asked for, and a row cap
        holds for poses and records alike): the dict also has "records", the chunk's records as a device-resident
        RecordWindow64 of that many rows -- what the filter was fed, row for row beside the poses
        (_ChunkedSession._with_records)."""
        planes, flags = self.pack_chunk(ev)
        buf = DeviceBuffer(planes.nbytes).upload(planes)
        return self.feed_planes(buf, planes.shape[0], flags, trajectory, records=records)

    def feed_planes(self, planes, n_events, flags=0, trajectory=False, offset=0, records=False):
        """n_events packed rows ([n_events][K] float4, or double4 for an FP64-event session) of the DeviceBuffer
        `planes`, starting `offset` bytes into it: row ranges of one resident plane are fed without copies.
        flags: EV_TIME_EVENTS if these rows hold time events (it may differ from chunk to chunk).
        records: as feed's."""
        K, f = self.batch, self.filters
        n_events, flags = int(n_events), int(flags) | self._form
        self._rows_in(planes, n_events, offset, K * (32 if self._form else 16))
        trajectory = self._records_trajectory(trajectory, records)
        tj = _Trajectory(chunk_trajectory_rows(trajectory, n_events) if trajectory is True else trajectory, n_events, K)
        win = _chunk_records(tj.rows, K) if records else None
        if records and tj.rows:   # (no rows: nothing to export, the launch is the one without records)
            check(lib.pekf_live_resume_rec_dev(K, n_events, planes.ptr + offset, self._init.ptr, self._t_init.ptr,
                                               self.alpha, f.X.ptr, f.P.ptr, *self._noise_args(), self._cnt.ptr,
                                               self._refs.ptr, flags, self._state.ptr, int(self._book["started"]),
                                               tj.traj.ptr, tj.dt.ptr, tj.rows, win.gd.ptr, win.am.ptr, win.my.ptr,
                                               None, None))
        else:
            # (a per-filter-noise filter: the same launch with its {q, r} plane in place of q and r)
            entry, noise = ((lib.pekf_live_resume_dev, (f.q, f.r)) if f.noise is None else
                            (lib.pekf_live_resume_noise_dev, (f.noise.ptr,)))
            check(entry(K, n_events, planes.ptr + offset, self._init.ptr, self._t_init.ptr, self.alpha,
                        f.X.ptr, f.P.ptr, *noise, self._cnt.ptr, self._refs.ptr, flags,
                        self._state.ptr, int(self._book["started"]), tj.traj.ptr if tj.rows else None,
                        tj.dt.ptr if tj.rows else None, tj.rows, None, None))
        out = self._after_launch(tj)
        if records:
            out = self._with_records(out, win)
        return out if tj.wanted else out[0]


class CalibrationSession:
    """Phase 1 fed in chunks (pekf_magcal_resume_dev): the phones' phase-1 messages as they arrive, a launch per
    chunk; the running sums, the message counts and each phone's first n_cal samples stay on the device between
    them (what the server's Magnetometer_Calibration object holds, KFS/Magnetometer_Calibration.cpp:7-36).

    Any cutting of a phase-1 plane into chunks -- single rows, empty chunks, a phone's message n_cal + 1 as a
    chunk's first or last row, phones that fire in different chunks or never -- gives
    calibrate_magnetometer(all the rows, n_cal, events)'s cal, fit and status bit for bit, for every phone and
    either event form, and after every chunk result() is that of the rows fed so far.  A phone's outputs are
    written in the chunk that holds its message n_cal + 1 and never again: its later messages do nothing.

    events: "f32" or "f64", fixed for the session; n_cal is fixed for the session too."""

    def __init__(self, batch, n_cal=100, events="f32"):
        if events not in EVENT_FORMS:
            raise ValueError("events must be 'f32' or 'f64'")
        K = self.batch = int(batch)
        self.n_cal, self.events = int(n_cal), events
        self._form = EV_F64_EVENTS if events == "f64" else 0
        nbytes = int(lib.pekf_magcal_state_bytes(K, self.n_cal, self._form))
        if nbytes < 0:
            raise ValueError("no phase-1 session state for batch=%d, n_cal=%d (n_cal must be in [6, 2^30))" % (K, self.n_cal))
        self._state, self._cal = DeviceBuffer(nbytes), DeviceBuffer(96 * K)
        self._fit, self._status = DeviceBuffer(48 * K), DeviceBuffer(4 * K)
        self.started = False
        self._last_times = np.zeros(K, np.int64)

    @property
    def device(self):
        """dict(cal, fit_dev, status_dev): the session's output buffers, what pekf_magcal_apply_dev reads"""
        return dict(cal=self._cal, fit_dev=self._fit, status_dev=self._status)

    def launch(self, ev_ptr, n_events, stream=None):
        """pekf_magcal_resume_dev on n_events rows at the device address ev_ptr (None with no rows), enqueued"""
        check(lib.pekf_magcal_resume_dev(self.batch, int(n_events), ev_ptr if n_events else None, self.n_cal,
                                         self._cal.ptr, self._fit.ptr, self._status.ptr, self._form, self._state.ptr,
                                         int(self.started), stream))
        self.started = True

    def feed(self, ev):
        """The next rows of every phone's phase-1 stream: a synth.generate_calibration_events-style dict of types
        (E, K), values (E, K, 3), times (E, K) and optionally values64; synth.EV_NONE where a phone has no message
        in a row.  Every message is a sample, whatever its type."""
        shape = np.asarray(ev["types"]).shape
        if len(shape) != 2 or shape[1] != self.batch:
            raise ValueError("phase1 is of %s phones, the session of %d" % (shape[1:], self.batch))
        if shape[0] == 0:
            return self.feed_planes(None, 0)
        # (f32: the chunk's first gap from the previous chunk's last times; phase 1 reads no time)
        buf, E, _ = _event_planes(dict(ev, t_init=self._last_times), self.events)
        self._last_times = np.asarray(ev["times"], np.int64)[-1].copy()
        return self.feed_planes(buf, E)

    def feed_planes(self, planes, n_events, offset=0):
        """n_events packed rows ([n_events][K] float4, or double4 for an FP64-event session) of the DeviceBuffer
        `planes`, starting `offset` bytes into it: row ranges of one resident plane are fed without copies."""
        n_events, offset = int(n_events), int(offset)
        _ChunkedSession._rows_in(planes, n_events, offset, self.batch * (32 if self._form else 16))
        self.launch(planes.ptr + offset if n_events else None, n_events)

    def recycle(self, columns):
        """The phones of `columns` (distinct indices in [0, K), any order) leave and the next ones start afresh
        (pekf_session_recycle_dev, its phase-1 group alone): sums and counts zero, outputs "not calibrated", as a
        new session's; their stored samples are unread until rewritten.  Every other column is untouched.  Either
        event form; an empty list launches nothing."""
        cols = _recycle_columns(columns, self.batch)
        if len(cols) == 0:
            return
        if not self.started:
            self.launch(None, 0)
        _launch_recycle(self.batch, cols, phase1_group=(self._state.ptr, self.n_cal, self._cal.ptr, self._fit.ptr,
                                                        self._status.ptr))

    def _group(self):
        return self._state.ptr, self.n_cal, self._cal.ptr, self._fit.ptr, self._status.ptr

    def export_columns(self, columns, release=True):
        """The phones of `columns` (recycle's rule) as a SessionColumns object: their sums, counts, stored samples
        and outputs in one device pack (pekf_session_export_dev, the phase-1 group alone) and, on f32 events,
        their rows of the last-times book.  release=True: the columns are then recycled -- the phones have left
        this session; release=False: they go on as they were (a fork).  Either event form."""
        cols = _recycle_columns(columns, self.batch)
        n = len(cols)
        pack = DeviceBuffer(SessionColumns.nbytes(n, self.n_cal, 0))
        if n and not self.started:
            self.launch(None, 0)
        if n:
            _launch_move(lib.pekf_session_export_dev, self.batch, cols, 0, pack, phase1_group=self._group())
        out = SessionColumns("calibration", pack, n, None, None, self.n_cal, self.events, np.zeros(n), np.zeros(n),
                             dict(last_times=self._last_times[cols].copy()))
        if release and n:
            self.recycle(cols)
        return out

    def import_columns(self, columns, pack):
        """The pack's phones (a CalibrationSession's export_columns, of the same n_cal and event form) into the
        listed columns, in the pack's order, overwriting what those columns held (pekf_session_import_dev).
        Refused, before any launch: another number of columns than the pack's, another n_cal or event form."""
        cols = _recycle_columns(columns, self.batch)
        _import_refusals(self, "calibration", cols, pack, ("n_cal", "events"))
        if len(cols) == 0:
            return
        if not self.started:
            self.launch(None, 0)
        _launch_move(lib.pekf_session_import_dev, self.batch, cols, 0, pack.pack, phase1_group=self._group())
        self._last_times[cols] = pack.book["last_times"]

    def result(self):
        """calibrate_magnetometer's dict (bias, W, fit, status, calibrated, cal, status_dev) from what has been
        fed so far; cal / status_dev are the session's own buffers, which later chunks write."""
        if not self.started:
            self.launch(None, 0)
        check(lib.pekf_device_sync())
        return _calibration_result(self.batch, self.device)


class PhoneSession(_ChunkedSession):
    """Live sessions from the phones' first message, fed as a server gets them: every chunk carries the next rows of
    the phase-2 plane and of the phase-3 plane (or the clients' wire frames), and costs two launches -- phase 2
    resumed (pekf_frontend_init_resume_dev), then phase 3 + the filter (pekf_live_join_dev) on phase 2's outputs
    in device memory.  Phones do not move in lock-step: in one chunk some still average, some get ready, some
    already filter; each filter joins the fused session by itself, in the chunk that holds its first phase-3
    message once it is ready.

    n_cal (None: no phase 1, the session above): the session calibrates from its own stream.  Every chunk may
    also carry the next rows of the phones' phase-1 plane (phase1 / planes1; feed_frames takes them from the
    frames), and the order within a chunk is: the phase-1 rows (pekf_magcal_resume_dev; always in the first
    chunk, later only when the chunk has such rows), pekf_magcal_apply_dev on the chunk's phase-2 and phase-3
    rows with the session's cal / status, phase 2 resumed, the join launch.  So a magnetometer message of
    phases 2 / 3 is corrected with what is known once its own chunk's phase-1 rows are in, where the one-shot
    session (run_session(..., calibration=calibrate_magnetometer(phase1, n_cal, events="f64")), for frames
    run_wire_session(frames, filters, calibration="frames", n_cal=n_cal)) corrects every one.  The session equals
    that one-shot bit for bit -- X, P, refs, ready, the summed counts, every trajectory row and record time, and
    session.calibration -- for every phone that has no phase-2 or phase-3 magnetometer message in a chunk BEFORE
    the chunk its fit fires in, and for every phone that never fires.  That is the client's own order: it
    finishes its calibration stage first.  A phone outside it has the magnetometer messages of those earlier
    chunks left as they came, which is what the server does (setValues and KFS/Parser.cpp:107 correct only once
    isCalibrated is set) and where this session differs from the one-shot one.

    For every phone whose phase-2 messages all come before its phase-3 messages (the client's own order), any
    cutting of the rows into chunks gives run_session(phase2, phase3, filters, events="f64") -- for frames
    run_wire_session(frames, filters) -- bit for bit: X, P, refs, ready, the summed counts and the concatenated
    trajectory / record_dt_ns / record_times_ns rows.  Outside that order: the phase-3 messages of a phone that
    is not ready are dropped, and phase-2 messages after a phone joined move only a t_init nobody reads.

    Sessions run on FP64 events (absolute times; pekf_live_join_dev takes nothing else).  filters: a BatchedEKF
    (FP64, AoS), as LiveSession's.  t_start (K,) int64: phase 2's start time (None: 0), with FP64 events only
    the t_init of a phone that never gets ready.

    A phone that leaves frees its column: recycle(columns) returns the listed columns to a new session's state in
    one launch, and the next phones' rows go into them while every other phone goes on."""

    # (a snapshot carries both device states, phase 2's and the fused kernel's, and phase 2's latest outputs)
    _BUFFERS = dict.fromkeys(("p2state", "state", "t_start", "init", "t_init", "ready", "refs"))
    _FIELDS = ("n_avg", "alpha")

    def __init__(self, filters, n_avg=100, alpha=0.1, t_start=None, n_cal=None):
        super().__init__(filters)
        K = self.batch
        self.n_avg, self.alpha = int(n_avg), float(alpha)
        self.n_cal = self._phase1 = None
        if n_cal is not None:   # phase 1's state and outputs: the snapshot carries them, and n_cal
            self.n_cal = int(n_cal)
            self._phase1 = p1 = CalibrationSession(K, self.n_cal, "f64")
            self._p1state, self._cal, self._fit, self._status = p1._state, p1._cal, p1._fit, p1._status
            self._BUFFERS = dict(self._BUFFERS, **dict.fromkeys(("p1state", "cal", "fit", "status")))
            self._FIELDS = self._FIELDS + ("n_cal",)
        t0 = np.zeros(K, np.int64) if t_start is None else np.ascontiguousarray(t_start, np.int64).reshape(K)
        n2, n3 = int(lib.pekf_frontend_init_state_bytes(K, EV_F64_EVENTS)), int(lib.pekf_live_state_bytes(K, EV_F64_EVENTS))
        if n2 < 0 or n3 < 0:
            raise ValueError("no session state for FP64 events")
        self._p2state, self._state = DeviceBuffer(n2), DeviceBuffer(n3)
        self._t_start, self._init, self._t_init = DeviceBuffer(8 * K), DeviceBuffer(48 * K), DeviceBuffer(8 * K)
        self._ready, self._cnt, self._refs = DeviceBuffer(4 * K), DeviceBuffer(4 * K), DeviceBuffer(48 * K)
        self._t_start.upload(t0)
        check(lib.pekf_memset(self._state.ptr, 0, self._state.nbytes, None))   # no filter has joined
        check(lib.pekf_device_sync())

    @classmethod
    def _from_snapshot(cls, filters, s):
        return cls(filters, s["n_avg"], s["alpha"], n_cal=s.get("n_cal"))

    def _feed_no_rows(self):
        self._launch(None, 0, None, 0, False, None)

    @property
    def calibration(self):
        """calibrate_magnetometer's dict as of the last chunk (a session with n_cal; otherwise None)"""
        if self._phase1 is None:
            return None
        if not self._book["started"]:
            self._feed_no_rows()
        check(lib.pekf_device_sync())
        return _calibration_result(self.batch, self._phase1.device)

    def _check_phase1(self, calibration, has_phase1):
        """The two refusals of a chunk's phase-1 arguments, before anything is packed or launched"""
        if self._phase1 is not None and calibration is not None:
            raise ValueError("a session constructed with n_cal calibrates from its own phase-1 rows: it takes no "
                             "calibration=")
        if self._phase1 is None and has_phase1:
            raise ValueError("phase-1 rows need a calibrating session: construct the session with n_cal=")

    def _pack(self, ev, name):
        """A chunk's rows of one phase -> (DeviceBuffer or None, rows)"""
        if ev is None:
            return None, 0
        shape = np.asarray(ev["types"]).shape
        if len(shape) != 2 or shape[1] != self.batch:
            raise ValueError("%s is of %s phones, the session of %d" % (name, shape[1:], self.batch))
        if shape[0] == 0:
            return None, 0
        planes = synth.pack_events64(ev, server_event_values(ev))
        return DeviceBuffer(planes.nbytes).upload(planes), shape[0]

    def feed(self, phase2=None, phase3=None, trajectory=False, calibration=None, phase1=None, records=False):
        """The next rows of the phase-2 plane and of the phase-3 plane: each a dict of types (E, K), values
        (E, K, 3), times (E, K) and optionally values64, synth.EV_NONE where a phone has no message in a row;
        either may be None or have no rows, and the two need not have the same number.  calibration:
        calibrate_magnetometer's dict; both chunks are corrected on the device first (pekf_magcal_apply_dev: per
        event, so it needs no state).  Returns (counts (K,) int32 records applied in this chunk, ready (K,) bool
        phase 2's state after it), and with trajectory (True or a row cap) a third value, the dict of trajectory /
        record_dt_ns / record_times_ns as LiveSession.feed's, rows counted within the chunk.
        phase1 (a session with n_cal only, which takes no calibration): the chunk's rows of the phase-1 plane, a
        dict of the same form; every message in it is a calibration sample, whatever its type.
        records=True (pekf_live_join_rec_dev): as LiveSession.feed's -- it implies a trajectory, and the dict gains
        "records", the chunk's RecordWindow64; in a calibrating session the corrected records, the server's Mag_1."""
        self._check_phase1(calibration, phase1 is not None)
        b1, E1 = self._pack(phase1, "phase1")
        b2, E2 = self._pack(phase2, "phase2")
        b3, E3 = self._pack(phase3, "phase3")
        return self._launch(b2.ptr if E2 else None, E2, b3.ptr if E3 else None, E3, trajectory, calibration,
                            b1.ptr if E1 else None, E1, records=records)

    def feed_planes(self, planes2, n2, planes3, n3, trajectory=False, calibration=None, offset2=0, offset3=0,
                    planes1=None, n1=0, offset1=0, records=False):
        """Row ranges of resident FP64 event planes ([rows][K] double4 DeviceBuffers), without copies: n2 rows of
        planes2 from byte offset2, n3 rows of planes3 from offset3 (offsets as LiveSession.feed_planes': inside the
        buffer, multiples of 16).  A buffer whose row count is 0 may be None.  calibration corrects the rows in
        place, so feed a row once.  planes1 / n1 / offset1 (a session with n_cal only): the chunk's rows of the
        phase-1 plane, in the same way; the session's own calibration corrects planes2 / planes3 in place too.
        records: as feed's."""
        self._check_phase1(calibration, planes1 is not None or int(n1) != 0)
        ptrs = []
        for planes, n, offset in ((planes2, int(n2), int(offset2)), (planes3, int(n3), int(offset3)),
                                  (planes1, int(n1), int(offset1))):
            self._rows_in(planes, n, offset, 32 * self.batch)
            ptrs.append(planes.ptr + offset if n else None)
        return self._launch(ptrs[0], int(n2), ptrs[1], int(n3), trajectory, calibration, ptrs[2], int(n1),
                            records=records)

    def feed_frames(self, frames_chunk, calibration=None, trajectory=False, records=False, refused="raise"):
        """The next [F][K][100] wire frames of the phones (wire.frames): parsed with a row per frame
        (wire_events(..., frame_rows=True): a frame's parse does not depend on earlier frames, and row f of each
        plane is frame f's message of that phase), then fed as feed_planes.  calibration: a dict, as feed;
        "frames" is refused -- without n_cal phase 1 is not chunked: calibrate first (calibrate_magnetometer), or
        construct the session with n_cal=, which then parses the chunk's phase-1 messages too
        (wire_events(..., phase1=True)) and feeds ev1's first E1 rows.  records: as feed's.
        refused: as wire_events.  "raise" (default): a frame the device parser does not take raises ValueError and
        the chunk is fed to nobody.  "repair": the chunk is repaired as wire_events does it, and the returned tuple
        gains two trailing items, bad_frame (K,) int32 -- -1, or the frame of THIS chunk that stopped the phone --
        and repaired (K,) bool.  A phone that stops is marked in the session (session.stopped): its connection has
        ended, as the server's process for it would have, so on every later feed_frames (in either mode) its
        column is no-message rows in every plane, whatever the phone goes on sending, and its bad_frame is -1;
        recycle(columns) clears the mark for the column's next phone, export_columns / import_columns / move and
        snapshot / restore carry it.  feed and feed_planes take planes, not frames, and know nothing of it."""
        _check_refused(refused)
        if isinstance(calibration, str) and self._phase1 is None:
            raise ValueError("a chunked session takes calibrate_magnetometer's dict: phase 1 from the frames "
                             "(calibration='frames') is not chunked in this session -- construct the session with "
                             "n_cal=")
        self._check_phase1(calibration, False)
        F, Kf = _frames_shape(frames_chunk)
        if Kf != self.batch:
            raise ValueError("the frames are of %d phones, the session of %d" % (Kf, self.batch))
        if F == 0:
            out = self._launch(None, 0, None, 0, trajectory, calibration, records=records)
            if refused == "repair":
                out += (np.full(self.batch, -1, np.int32), np.zeros(self.batch, bool))
            return out
        stopped = self._book.get("stopped")
        if self._phase1 is not None:
            w = wire_events(frames_chunk, None, True, phase1=True, refused=refused, stopped=stopped)
            out = self.feed_planes(w["ev2"], w["E2"], w["ev3"], w["E3"], trajectory, None,
                                   offset3=32 * self.batch * w["ev3_from"], planes1=w["ev1"], n1=w["E1"],
                                   records=records)
        else:
            w = wire_events(frames_chunk, None, True, refused=refused, stopped=stopped)
            out = self.feed_planes(w["ev2"], w["E2"], w["ev3"], w["E3"], trajectory, calibration,
                                   offset3=32 * self.batch * w["ev3_from"], records=records)
        if refused == "repair":
            self._book["stopped"] = self.stopped | (w["bad_frame"] >= 0)
            out += (w["bad_frame"], w["repaired"])
        return out

    @property
    def stopped(self):
        """(K,) bool, a copy: the phones whose stream a frame ended (feed_frames(refused="repair")) and whose column
        has not been recycled since"""
        return np.array(self._book.get("stopped", np.zeros(self.batch, bool)), bool)

    def _launch(self, ev2, E2, ev3, E3, trajectory, calibration, ev1=None, E1=0, records=False):
        K, f = self.batch, self.filters
        if self._phase1 is not None:   # the chunk's phase-1 rows first: its other rows are corrected with the result
            if E1 or not self._book["started"]:
                self._phase1.started = self._book["started"]   # (the book is what a snapshot carries)
                self._phase1.launch(ev1, E1)
            calibration = self._phase1.device
        if calibration is not None:
            if E2:
                _apply_calibration(calibration, K, E2, ev2, EV_F64_EVENTS)
            if E3:
                _apply_calibration(calibration, K, E3, ev3, EV_F64_EVENTS)
        check(lib.pekf_frontend_init_resume_dev(K, E2, ev2, self._t_start.ptr, self.n_avg, self._init.ptr,
                                                self._t_init.ptr, self._ready.ptr, EV_F64_EVENTS, self._p2state.ptr,
                                                int(self._book["started"]), None))
        trajectory = self._records_trajectory(trajectory, records)
        tj = _Trajectory(chunk_trajectory_rows(trajectory, E3) if trajectory is True else trajectory, E3, K)
        win = _chunk_records(tj.rows, K) if records else None
        # (no rows: any valid pointer, none is read)
        if records and tj.rows:   # (no trajectory rows: nothing to export, the launch is the one without records)
            check(lib.pekf_live_join_rec_dev(K, E3, ev3 if E3 else self._state.ptr, self._init.ptr, self._t_init.ptr,
                                             self.alpha, f.X.ptr, f.P.ptr, *self._noise_args(), self._cnt.ptr,
                                             self._refs.ptr, EV_F64_EVENTS, self._state.ptr, tj.traj.ptr, tj.dt.ptr,
                                             tj.rows, win.gd.ptr, win.am.ptr, win.my.ptr, None, None))
        else:
            entry, noise = ((lib.pekf_live_join_dev, (f.q, f.r)) if f.noise is None else
                            (lib.pekf_live_join_noise_dev, (f.noise.ptr,)))   # (per-filter noise: its {q, r} plane)
            check(entry(K, E3, ev3 if E3 else self._state.ptr, self._init.ptr, self._t_init.ptr,
                        self.alpha, f.X.ptr, f.P.ptr, *noise, self._cnt.ptr, self._refs.ptr,
                        EV_F64_EVENTS, self._state.ptr, tj.traj.ptr if tj.rows else None,
                        tj.dt.ptr if tj.rows else None, tj.rows, None, None))
        out = self._after_launch(tj)
        if records:
            out = self._with_records(out, win)
        return out[:1] + (self._ready.download((K,), np.int32).astype(bool),) + out[1:]

    def _first_records(self, first):
        # a phone's record times start from the t_init of the chunk in which it applies its first record
        if first.any():
            self._book["t_init"] = np.where(first, self._t_init.download((self.batch,), np.int64), self._book["t_init"])

    def recycle(self, columns, t_start=None, X0=None, P0=None, final=False, q=None, r=None):
        """The phones of `columns` leave and the next ones start afresh (pekf_session_recycle_dev, one launch): each
        listed column returns to the state a brand-new session gives it -- calibration (a session with n_cal),
        phase 2 and the filter -- and every other column goes on as if nothing had happened.  Fed a new phone's
        rows, a recycled column equals, bit for bit, a new PhoneSession fed those rows; it is what the server does
        per connection (one client per process, a new Parser for the next).  Valid at any chunk boundary, before
        the first chunk included.

        columns: a 1-D sequence of distinct integer indices in [0, K), in any order; an empty one launches nothing
        and changes nothing.  t_start (n,) int64: the new phones' phase-2 start times, as the constructor's (None:
        0).  X0 (n, 4) / P0 (n, 4, 4): the filters the new phones start from (both or neither; None: X = [1,0,0,0],
        P = I, BatchedEKF.reset's).  final=True returns dict(X (n, 4), P (n, 4, 4), total_counts (n,)) of the
        departing phones, in the order of `columns` -- their last poses from the same launch, not a download of
        every column; otherwise None.  The columns' total_counts and record times start again.
        q, r (a per-filter-noise filter only; both or neither): the new phones' noise, scalars or (n,) values,
        validated as BatchedEKF's and written into those entries of filters.noise (BatchedEKF.set_noise) before
        the recycle launch -- the one point at which a live column's noise may change, since its filter starts
        afresh.  None: the columns keep the noise they had.

        LiveSession has no recycle: its lanes start from one launch-wide `resume` word, and a per-lane fresh start
        there needs the joining kernels on f32 events, which do not exist."""
        K = self.batch
        cols = _recycle_columns(columns, K)
        n = len(cols)
        if (X0 is None) != (P0 is None):
            raise ValueError("X0 needs P0 (and P0 needs X0)")
        if (q is None) != (r is None):
            raise ValueError("q needs r (and r needs q)")
        if q is not None:
            if self.filters.noise is None:
                raise ValueError("recycle(q=, r=) needs a per-filter-noise filter: construct BatchedEKF with array "
                                 "q / r (a scalar-noise filter has one q and one r for every column)")
            q, r = _noise_arrays(q, r, n, "listed column")
        for name, a, shape in (("t_start", t_start, (n,)), ("X0", X0, (n, 4)), ("P0", P0, (n, 4, 4))):
            if a is not None and np.shape(a) != shape:
                raise ValueError("%s must have shape %s for %d columns" % (name, shape, n))
        if n == 0:
            return dict(X=np.zeros((0, 4)), P=np.zeros((0, 4, 4)), total_counts=np.zeros(0, np.int64)) if final else None
        if not self._book["started"]:
            self._feed_no_rows()   # the buffers in their started form (as refs does)
        t0 = np.zeros(n, np.int64) if t_start is None else np.ascontiguousarray(t_start, np.int64)
        # the entry's optional per-column arrays: X0, P0, final_X, final_P, t_start_new
        bufs = [None if X0 is None else DeviceBuffer(32 * n).upload(f64(X0, (n, 4))),
                None if P0 is None else DeviceBuffer(128 * n).upload(f64(P0, (n, 4, 4))),
                DeviceBuffer(32 * n) if final else None, DeviceBuffer(128 * n) if final else None,
                None if t_start is None else DeviceBuffer(8 * n).upload(t0)]
        ptr = [b.ptr if b is not None else None for b in bufs]
        f = self.filters
        if q is not None:
            f.set_noise(cols, q, r)
        p1 = None
        if self._phase1 is not None:
            p1 = (self._p1state.ptr, self.n_cal, self._cal.ptr, self._fit.ptr, self._status.ptr)
        _launch_recycle(K, cols, (self._state.ptr, f.X.ptr, f.P.ptr, self._refs.ptr) + tuple(ptr[:4]),
                        (self._p2state.ptr, self._t_start.ptr, self._init.ptr, self._t_init.ptr, self._ready.ptr, ptr[4]),
                        p1)
        book = self._book
        out = None
        if final:
            out = dict(X=bufs[2].download((n, 4), np.float64), P=bufs[3].download((n, 4, 4), np.float64),
                       total_counts=book["total_counts"][cols].copy())
        book["total_counts"][cols] = 0
        book["dt_sum"][cols] = 0.0
        book["t_init"][cols] = t0
        if "stopped" in book:   # the next phone's connection is a new one
            book["stopped"][cols] = False
        return out

    _BOOK_ROWS = ("t_init", "dt_sum", "total_counts")

    def _move_groups(self):
        """the session's three groups as _launch_move takes them (phase 1: a session with n_cal only)"""
        f, p1 = self.filters, None
        if self._phase1 is not None:
            p1 = (self._p1state.ptr, self.n_cal, self._cal.ptr, self._fit.ptr, self._status.ptr)
        return ((self._state.ptr, f.X.ptr, f.P.ptr, self._refs.ptr),
                (self._p2state.ptr, self._t_start.ptr, self._init.ptr, self._t_init.ptr, self._ready.ptr), p1)

    def export_columns(self, columns, release=True):
        """The live phones of `columns` (recycle's rule: distinct indices in [0, K), any order) as a SessionColumns
        object, in that order: everything the session holds for them on the device -- the calibration state and
        outputs (a session with n_cal), phase 2's, the filter's with X, P and refs -- gathered into one pack by
        one launch (pekf_session_export_dev), their q and r, and their rows of the host book.  Valid at any chunk
        boundary, before the first chunk included (the session's zero-row launch runs first, as recycle's).
        release=True: the listed columns are then recycled (recycle's own launch and book reset): the phones have
        left this session, and import_columns brings them into free columns of this or another session, of any
        batch -- a compaction, or through to_host / from_host a move to another device.  release=False: the
        columns go on as they were, and the object is a fork of them.  An empty list launches nothing."""
        K, f = self.batch, self.filters
        cols = _recycle_columns(columns, K)
        n = len(cols)
        pack = DeviceBuffer(SessionColumns.nbytes(n, self.n_cal, EV_F64_EVENTS))
        if n:
            if not self._book["started"]:
                self._feed_no_rows()
            _launch_move(lib.pekf_session_export_dev, K, cols, EV_F64_EVENTS, pack, *self._move_groups())
        q, r = (np.full(n, f.q), np.full(n, f.r)) if f.noise is None else (f.q[cols].copy(), f.r[cols].copy())
        out = SessionColumns("phone", pack, n, self.n_avg, self.alpha, self.n_cal, "f64", q, r,
                             dict({name: self._book[name][cols].copy() for name in self._BOOK_ROWS},
                                  stopped=self.stopped[cols]))
        if release and n:
            self.recycle(cols)
        return out

    def import_columns(self, columns, pack):
        """The pack's phones (export_columns' SessionColumns, of this or another PhoneSession) into the listed
        columns, in the pack's order, overwriting whatever those columns held (pekf_session_import_dev, one
        launch); their book rows become the pack's.  Fed its next rows in its new column, a phone goes on bit
        for bit as in the column it left: X, P, refs, ready, the counts, every trajectory row and record time,
        the calibration.  Every other column is untouched.
        Refused with ValueError, before any launch: columns that break recycle's rule or are not pack.n; a pack
        whose n_avg, alpha or n_cal is not the session's (phase 1 on one side only included); noise that does not
        fit -- the session state holds the covariance scaled by the column's r (BatchedEKF's docstring), so a
        phone keeps its q and r: a per-filter-noise filter takes the pack's pairs into its plane
        (BatchedEKF.set_noise), a scalar filter accepts only pairs equal to its own q and r."""
        K, f = self.batch, self.filters
        cols = _recycle_columns(columns, K)
        _import_refusals(self, "phone", cols, pack, ("n_avg", "alpha", "n_cal"))
        if f.noise is None:
            if not (np.all(pack.q == f.q) and np.all(pack.r == f.r)):
                raise ValueError("the pack's phones run with their own q and r, which are not this scalar-noise "
                                 "filter's (q=%r, r=%r): import into a per-filter-noise filter" % (f.q, f.r))
        else:
            _noise_arrays(pack.q, pack.r, pack.n, "listed column")
        if len(cols) == 0:
            return
        if not self._book["started"]:
            self._feed_no_rows()
        if f.noise is not None:
            f.set_noise(cols, pack.q, pack.r)
        _launch_move(lib.pekf_session_import_dev, K, cols, EV_F64_EVENTS, pack.pack, *self._move_groups())
        for name in self._BOOK_ROWS:
            self._book[name][cols] = pack.book[name]
        stopped = self.stopped   # (a pack from before the mark existed: none stopped)
        stopped[cols] = pack.book.get("stopped", False)
        if stopped.any() or "stopped" in self._book:
            self._book["stopped"] = stopped

    def move(self, src, dst):
        """import_columns(dst, export_columns(src)) within this session: the phones of src go on in the columns
        dst (as many; dst[i] takes src[i]) and the columns of src are recycled.  src and dst must be disjoint --
        a compaction moves phones into free columns; a permutation in place is refused, before any launch."""
        src, dst = _recycle_columns(src, self.batch), _recycle_columns(dst, self.batch)
        if len(src) != len(dst):
            raise ValueError("%d columns listed for a pack of %d" % (len(dst), len(src)))
        if len(np.intersect1d(src, dst)):
            raise ValueError("src and dst overlap: a phone moves into a free column (no permutation in place)")
        self.import_columns(dst, self.export_columns(src))


class SessionLog:
    """The server's log (KalmanFilter::WriteTextFile, logformat's format) of the listed columns of a chunked
    session, written chunk by chunk from the chunks fed with records=True: the replayable trace main_file.py runs
    from, byte for byte logformat.write_log of the whole session's arrays.

    session: a LiveSession or PhoneSession; columns: distinct column indices (recycle's rule); paths: a file per
    column.  append(result) takes a chunk's returned dict (the last value feed / feed_planes / feed_frames
    return).  A column's header -- mag_0 / acc_0 from the session's refs, the three identity lines, and the
    phone's t_init as the T before its first record's T -- is written when its first record arrives, so a phone
    with no record gets no file; then per record gyro, T (record_times_ns), q_gyro (records.gyro_chain from the
    column's own q_gyro of its last record so far: the identity at first, then row count - 1 of the previous
    chunk -- not the kernel's final value, which has run over rows the chunk did not write), Mag_1, Acc_1, X_k
    (the chunk's trajectory row) and Wahba_quart (records.wahba_quaternions(), main_file.py:40's 0.5 / 0.5).
    Every chunk in which a listed column applies a record must be appended, in order; a column that is recycled
    or moved starts another phone's log: make a new SessionLog for it."""

    def __init__(self, session, columns, paths):
        self.session, self.columns = session, _recycle_columns(columns, session.batch)
        self.paths = [os.fspath(p) for p in paths]
        if len(self.paths) != len(self.columns):
            raise ValueError("%d paths for %d columns" % (len(self.paths), len(self.columns)))
        self._q = np.tile([1.0, 0.0, 0.0, 0.0], (session.batch, 1))
        self._begun = np.zeros(len(self.columns), bool)

    def append(self, result):
        from . import logformat
        cols = self.columns
        win = result.get("records") if isinstance(result, dict) else None
        if win is None:
            raise ValueError("SessionLog.append takes the dict of a chunk fed with records=True (a chunk fed without "
                             "records cannot be logged, and the record times are NaN from there on)")
        if (np.asarray(win.chunk_counts)[cols] > win.window).any():
            raise ValueError("the chunk's row cap (%d rows) cut a listed column's records: they were applied but "
                             "not exported, and the record times are NaN from there on" % win.window)
        counts = np.asarray(win.counts)
        if len(cols) == 0 or win.window == 0 or not counts[cols].any():
            return
        wahba = win.wahba_quaternions()
        q_gyro = win.gyro_chain(self._q, want_traj=True)[1]
        gyro, _, acc, mag, refs = win.download_filters(cols)
        t_init = self.session._book["t_init"]
        for i, k in enumerate(cols):
            n = int(counts[k])
            if n == 0:
                continue
            times = [t_init[k]] * (not self._begun[i]) + list(result["record_times_ns"][:n, k])
            with open(self.paths[i], "a" if self._begun[i] else "w") as fh:
                logformat.write_log(fh, times, gyro[:n, i], acc[:n, i], mag[:n, i], refs[i, :3], refs[i, 3:],
                                    q_gyro[:n, k], result["trajectory"][:n, k], wahba[:n, k],
                                    continued=bool(self._begun[i]))
            self._begun[i] = True
            self._q[k] = q_gyro[n - 1, k]


class FilterHandle:
    """B KalmanFilter objects behind one native handle (pekf_filter_*).

    The handle owns what the reference object owns (ExtendedKalmanFilter.py:6-15): the Wahba
    reference (acc0, mag0), Q = q I, R = r I and previousT, plus the state X, P, which stays in
    device memory.  `update` is one main_file.py:42-45 iteration for every filter from FP64
    host arrays (online serving); `run` advances the same state through a resident stream window.
    """

    def __init__(self, acc0, mag0, q=1.0, r=0.1, t0_ns=None, precision="f64", layout="aos"):
        acc0 = np.ascontiguousarray(acc0, np.float64).reshape(-1, 3)
        mag0 = np.ascontiguousarray(mag0, np.float64).reshape(-1, 3)
        self.batch = acc0.shape[0]
        assert mag0.shape[0] == self.batch
        t0 = None if t0_ns is None else np.ascontiguousarray(t0_ns, np.int64).reshape(self.batch)
        h = ctypes.c_void_p()
        check(lib.pekf_filter_create(self.batch, acc0.ctypes.data, mag0.ctypes.data, float(q), float(r),
                                     t0.ctypes.data if t0 is not None else None, _run_flags(precision, layout),
                                     ctypes.byref(h)))
        self.h = h.value

    def update(self, gyro, t_ns, acc, mag, missing=None, want_x=True):
        """One record per filter: Prediction(gyro, t_ns) + Correction(mag, acc). Returns X (B, 4)."""
        B = self.batch
        g, a, m = (np.ascontiguousarray(v, np.float64).reshape(B, 3) for v in (gyro, acc, mag))
        t = np.ascontiguousarray(t_ns, np.int64).reshape(B)
        miss = None if missing is None else np.ascontiguousarray(missing, np.uint8).reshape(B)
        X = np.empty((B, 4)) if want_x else None
        check(lib.pekf_filter_update(self.h, g.ctypes.data, t.ctypes.data, a.ctypes.data, m.ctypes.data,
                                     miss.ctypes.data if miss is not None else None,
                                     X.ctypes.data if X is not None else None))
        return X

    def run(self, win: IMUWindow, n_steps=None, step0=0, want_traj=False, counts=None):
        """pekf_filter_run over a resident window (the window's refs are not used: the handle's are)."""
        n_steps = win.window if n_steps is None else int(n_steps)
        assert win.batch == self.batch
        tb = DeviceBuffer(32 * n_steps * self.batch) if want_traj else None
        cb = _launch_counts(win, counts, n_steps, step0)
        check(lib.pekf_filter_run_ext(self.h, n_steps, win.window, int(step0), win.gd.ptr, win.am.ptr, win.my.ptr,
                                      win.dtx.ptr if win.dtx is not None else None,
                                      tb.ptr if tb is not None else None, cb.ptr if cb is not None else None, None))
        check(lib.pekf_device_sync())
        return tb.download((n_steps, self.batch, 4), np.float64) if want_traj else None

    def set_state(self, X=None, P=None):
        Xa = None if X is None else f64(X, (self.batch, 4))
        Pa = None if P is None else f64(P, (self.batch, 4, 4))
        check(lib.pekf_filter_set_state(self.h, Xa.ctypes.data if Xa is not None else None,
                                        Pa.ctypes.data if Pa is not None else None))

    def get_state(self):
        X, P = np.empty((self.batch, 4)), np.empty((self.batch, 4, 4))
        check(lib.pekf_filter_get_state(self.h, X.ctypes.data, P.ctypes.data))
        return X, P

    def set_time(self, t_ns):
        t = np.ascontiguousarray(t_ns, np.int64).reshape(self.batch)
        check(lib.pekf_filter_set_time(self.h, t.ctypes.data))

    def get_time(self):
        """previousT of every filter (B,) int64 ns (KalmanFilter.previousT)."""
        t = np.empty(self.batch, np.int64)
        check(lib.pekf_filter_get_time(self.h, t.ctypes.data))
        return t

    def close(self):
        if getattr(self, "h", None):
            lib.pekf_filter_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------ batched per-call operators
# NumPy-level wrappers over the host-pointer entry points (one GPU thread per item).

def _in(a, shape):
    """Read-only C-contiguous float64 view of an input (copied only if it is not one already):
    the host-pointer entry points never write their inputs."""
    return np.ascontiguousarray(a, dtype=np.float64).reshape(shape)


def _n(a, k):
    return np.size(a) // k


def _p(a):
    return a.ctypes.data


def rk4(q0, dt_ns, w):
    n = _n(q0, 4)
    q0, dt, w = _in(q0, (n, 4)), _in(dt_ns, (n,)), _in(w, (n, 3))
    out = np.empty((n, 4))
    check(lib.pekf_rk4(n, _p(q0), _p(dt), _p(w), _p(out)))
    return out


def norm(a):
    """Row norms of a (n, len) array, sequential sum of squares (UtilityFunctions.py:16-21)."""
    a = np.atleast_2d(np.ascontiguousarray(a, dtype=np.float64))
    n, k = a.shape
    out = np.empty(n)
    check(lib.pekf_norm(n, k, _p(a), _p(out)))
    return out


def jacobian_a(w):
    n = _n(w, 3)
    w = _in(w, (n, 3))
    out = np.empty((n, 4, 4))
    check(lib.pekf_jacobian_a(n, _p(w), _p(out)))
    return out


def jacobian_b(q):
    n = _n(q, 4)
    q = _in(q, (n, 4))
    out = np.empty((n, 4, 3))
    check(lib.pekf_jacobian_b(n, _p(q), _p(out)))
    return out


def comparator(q1, q2):
    n = _n(q1, 4)
    a, b = _in(q1, (n, 4)), _in(q2, (n, 4))
    out = np.empty((n, 4))
    check(lib.pekf_comparator(n, _p(a), _p(b), _p(out)))
    return out


def predict(gyro, dt_ns, X, P, Q, R):
    n = _n(X, 4)
    args = (_in(gyro, (n, 3)), _in(dt_ns, (n,)), _in(X, (n, 4)), _in(P, (n, 4, 4)),
            _in(Q, (n, 3, 3)), _in(R, (n, 4, 4)))
    z, Pm, K = np.empty((n, 4)), np.empty((n, 4, 4)), np.empty((n, 4, 4))
    check(lib.pekf_predict(n, *[_p(a) for a in args], _p(z), _p(Pm), _p(K)))
    return z, Pm, K


def correct(mag, acc, z, P, K, acc0, mag0):
    n = _n(z, 4)
    args = (_in(mag, (n, 3)), _in(acc, (n, 3)), _in(z, (n, 4)), _in(P, (n, 4, 4)), _in(K, (n, 4, 4)),
            _in(acc0, (n, 3)), _in(mag0, (n, 3)))
    X, Po = np.empty((n, 4)), np.empty((n, 4, 4))
    check(lib.pekf_correct(n, *[_p(a) for a in args], _p(X), _p(Po)))
    return X, Po


def _wahba(fn, k, acc0, mag0, acc, mag, k_acc, k_mag):
    n = _n(acc, 3)
    args = (_in(acc0, (n, 3)), _in(mag0, (n, 3)), _in(acc, (n, 3)), _in(mag, (n, 3)),
            _in(k_acc, (n,)), _in(k_mag, (n,)))
    out = np.empty((n,) + k)
    check(fn(n, *[_p(a) for a in args], _p(out)))
    return out


def wahba_rotation(acc0, mag0, acc, mag, k_acc, k_mag):
    return _wahba(lib.pekf_wahba_rotation, (3, 3), acc0, mag0, acc, mag, k_acc, k_mag)


def wahba_quaternion(acc0, mag0, acc, mag, k_acc, k_mag):
    return _wahba(lib.pekf_wahba_quaternion, (4,), acc0, mag0, acc, mag, k_acc, k_mag)


def quat_to_rpy(q):
    """UtilityFunctions.Quart2RPY for each row of q (n,4): roll, pitch, yaw in degrees."""
    n = _n(q, 4)
    q = _in(q, (n, 4))
    out = np.empty((n, 3))
    check(lib.pekf_quat_to_rpy(n, _p(q), _p(out)))
    return out


def rotmat_to_quat(M):
    n = _n(M, 9)
    M = _in(M, (n, 3, 3))
    out = np.empty((n, 4))
    check(lib.pekf_rotmat_to_quat(n, _p(M), _p(out)))
    return out
