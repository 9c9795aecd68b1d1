"""Exact phase-3 chains for the items of tests/frontend_families.py, and the error of the reference's own float64
statement against them (needs mpmath; no GPU, no reference checkout):

    python tests/golden/make_frontend_golden.py

For each item the whole of Parser::ExecuteKalmanFilter's arithmetic is run at DPS = 80 digits from the doubles as
they are: the state machine (Parser.cpp:148-219, restated here and required to give the tuples the families module
hands out), the interpolation v = y1 + (y2 - y1) (t3 - t1) / (t2 - t1) (:259-267), the normalisation v / |v|
(:221-228) and the low-pass l <- alpha x + beta l from zero (KalmanFilter.cpp:279-303), alpha and beta the two
doubles the reference and the device both multiply by (beta = the double 1.0 - alpha: a coefficient of the
recurrence, not a rounding of it -- taken as the real 1 - alpha it would charge both of them 5e-17 / alpha).

Stored, for the set "f64" (nine families of 32 items and the 8 judged apart) and the set "f32" (the same with every
sample rounded to float32; scale's 1e-80 and 1e80 items left out), the items side by side in
frontend_families.stacked()'s order -- the inputs come from the generator and are not stored:
  <set>_count     (n,) int16        the item's records
  <set>_kappa     (n,)              (|y1| + |lam| |y2 - y1|) / |v| of the last record's judged channel (lowpass: the
                                    largest of that channel's records); NaN for the items judged apart
  <set>_rho       (n,)              |out - exact|_max / (kappa U) of oracle.frontend_numpy.run_frontend on that
                                    record and channel; NaN for the items judged apart
  <set>_Y         (9,)              each family's largest rho, at least 1
and per stored row (a record of an item; every record, but of a lowpass item the LOWPASS_KEPT of its 200 -- all of
them would be 1 MiB):
  <set>_row_item  (N,) int16, <set>_row_rec (N,) int16   the item and the record's index
  <set>_out       (N, 2, 3)         the exact low-pass output {acc, mag}, each value rounded once
  <set>_res       (N, 2, 3) float32 exact - out
  <set>_kappa_row (N, 2) float32    kappa of that record in each channel (lowpass: the largest up to that record)
  <set>_nan       (N, 2, 3) bool    the reference's output is NaN there (only on items judged apart, whose judged
                                    channel has out = res = kappa_row = NaN)

Output: tests/golden/frontend_families.npz
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("PEKF_GOLDEN_OUT") or HERE
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

import mpmath as mp  # noqa: E402

from oracle import frontend_numpy as fe  # noqa: E402
from tests import frontend_families as ff  # noqa: E402

DPS = 80
LOWPASS_KEPT = (0, 1, 2, 3, 7, 15, 31, 63, 127) + tuple(range(ff.LOWPASS_RECORDS - 7, ff.LOWPASS_RECORDS + 1))


def machine(item):
    """Parser::WriteKalmanFilterMeasurement -> per record ((t1, t2, t3, y1, y2) of acc, of mag)"""
    acc0, t_acc0, mag0, t_mag0 = item["init_acc"], item["t_init"], item["init_mag"], item["t_init"]
    acc1 = mag1 = None
    t_acc1 = t_mag1 = t_gyro = 0
    gyro_set = acc1_set = mag1_set = False
    out = []
    for ty, v, t in zip(item["types"], item["values"], item["times"]):
        ty, t = int(ty), int(t)
        if ty == ff.GYRO:
            if gyro_set:
                if acc1_set:
                    acc0, t_acc0 = acc1, t_acc1
                if mag1_set:
                    mag0, t_mag0 = mag1, t_mag1
                acc1_set = mag1_set = False
            t_gyro, gyro_set = t, True
        elif ty == ff.ACC:
            if gyro_set:
                acc1, t_acc1, acc1_set = v, t, True
            else:
                acc0, t_acc0 = v, t
        elif ty == ff.MAG:
            if gyro_set:
                mag1, t_mag1, mag1_set = v, t, True
            else:
                mag0, t_mag0 = v, t
        if acc1_set and mag1_set:
            out.append(((t_acc0, t_acc1, t_gyro, acc0, acc1), (t_mag0, t_mag1, t_gyro, mag0, mag1)))
            acc0, t_acc0, mag0, t_mag0 = acc1, t_acc1, mag1, t_mag1
            gyro_set = acc1_set = mag1_set = False
    return out


def _norm(v):
    return mp.sqrt(sum(x * x for x in v))


def exact_channel(tups, alpha):
    """One channel's records at DPS digits -> [(low-pass output (3 mpf), kappa)]"""
    a, b = mp.mpf(alpha), mp.mpf(1.0 - alpha)
    low, out = [mp.mpf(0)] * 3, []
    for t1, t2, t3, y1, y2 in tups:
        y1, y2 = [mp.mpf(float(x)) for x in y1], [mp.mpf(float(x)) for x in y2]
        lam = mp.mpf(t3 - t1) / mp.mpf(t2 - t1)
        v = [p + (q - p) * lam for p, q in zip(y1, y2)]
        nv = _norm(v)
        kappa = (_norm(y1) + abs(lam) * _norm([q - p for p, q in zip(y1, y2)])) / nv
        low = [a * x / nv + b * l for x, l in zip(v, low)]
        out.append((low, kappa))
    return out


def solve_set(items, sl):
    n = len(items)
    count, kappa, rho = np.zeros(n, np.int16), np.full(n, np.nan), np.full(n, np.nan)
    rows = dict(item=[], rec=[], out=[], res=[], kappa=[], nan=[])
    for i, it in enumerate(items):
        is_apart = i >= sl["apart"].start
        tups = machine(it)
        theirs = ff.tuples(it)
        assert len(tups) == len(theirs)
        for mine, (_, _, a, m) in zip(tups, theirs):
            for x, y in zip(mine, (a, m)):
                assert x[:3] == y[:3] and all(np.array_equal(x[j], y[j], equal_nan=True) for j in (3, 4))
        count[i] = len(tups)
        ch = it["ch"]
        chans = [None if is_apart and c == ch else exact_channel([t[c] for t in tups], it["alpha"]) for c in (0, 1)]
        ref = fe.run_frontend(it["types"], it["values"], it["times"], it["init_acc"], it["init_mag"], it["t_init"], it["alpha"])
        ref = np.stack([ref[2], ref[3]], axis=1)          # (R, 2, 3)
        assert is_apart or np.isfinite(ref).all()
        lowpass = it["alpha"] != 1.0
        keep = [r for r in range(len(tups)) if not lowpass or r in LOWPASS_KEPT or r == len(tups) - 1]
        run = [mp.mpf(0), mp.mpf(0)]
        for r in range(len(tups)):
            o, e, k = np.full((2, 3), np.nan), np.full((2, 3), np.nan, np.float32), np.full(2, np.nan, np.float32)
            for c in (0, 1):
                if chans[c] is None:
                    continue
                low, kap = chans[c][r]
                run[c] = max(run[c], kap) if lowpass else kap
                o[c] = [float(x) for x in low]
                e[c] = [float(x - mp.mpf(float(x))) for x in low]
                k[c] = float(run[c])
            if r in keep:
                rows["item"].append(i); rows["rec"].append(r); rows["out"].append(o); rows["res"].append(e)
                rows["kappa"].append(k); rows["nan"].append(np.isnan(ref[r]))
        if not is_apart:
            low, _ = chans[ch][-1]
            kappa[i] = float(run[ch])
            err = max(abs(mp.mpf(float(x)) - y) for x, y in zip(ref[-1, ch], low))
            rho[i] = float(err / (run[ch] * mp.mpf(ff.U)))
    Y = np.array([max(1.0, float(rho[sl[name]].max())) for name in ff.NAMES])
    return dict(count=count, kappa=kappa, rho=rho, Y=Y, row_item=np.array(rows["item"], np.int16),
                row_rec=np.array(rows["rec"], np.int16), out=np.array(rows["out"]), res=np.array(rows["res"], np.float32),
                kappa_row=np.array(rows["kappa"], np.float32), nan=np.array(rows["nan"], bool))


def main():
    mp.mp.dps = DPS
    store = {}
    for which in ("f64", "f32"):
        items, sl = ff.stacked(which)
        for k, v in solve_set(items, sl).items():
            store["%s_%s" % (which, k)] = v
    path = os.path.join(OUT, "frontend_families.npz")
    np.savez_compressed(path, **store)
    print("frontend_families.npz %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
