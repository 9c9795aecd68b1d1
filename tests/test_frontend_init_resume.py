"""Phase 2 fed in chunks (pekf_frontend_init_resume_dev, pekf_frontend_init_state_bytes): however the rows of a
phase-2 plane are cut into launches, init, t_init and ready have the bits of the one launch.

The yardstick is the existing one-launch kernel, which is not under test: engine.frontend_init(..., stats=False)
for the whole plane, and pekf_frontend_init_ext_dev with stats = NULL on the first n rows of the same resident
plane for what every chunk must leave behind.  NaNs (the means of a phone that is not ready) are compared by
position.  Forms: f32 events (time events honoured) and FP64 events.  The reference parser's own phase-2 trace
(tests/golden/parser.npz) is fed in chunks of 3 and must give the fixture's bits."""
import numpy as np
import pytest

from poseestimationkf_amd import synth

from .test_parser_golden import SESSIONS, load_golden, phase_events, same_bits
from .test_parser_golden_gpu import _event_dict

pytestmark = pytest.mark.gpu

K, E, N_AVG = 70, 60, 5    # one full wave plus six lanes, ending inside an 8-lane group
FORMS = ["f32", "f64"]
OTHER, PAUSED = 3, 9       # the phone with type-3 messages; the phone whose clock pauses (f32: a time event)
PAUSE_ROW = 20


@pytest.fixture(scope="module")
def eng():
    from poseestimationkf_amd import engine
    from poseestimationkf_amd._lib import device_count
    assert device_count() > 0, "GPU tests need a HIP device"
    return engine


def _stream():
    ev = dict(synth.generate_events(np.arange(K), E, seed=31))
    ty, t = ev["types"].copy(), ev["times"].copy()
    ty[12:, np.arange(K) % 6 == 1] = synth.EV_NONE       # short streams: these phones never get ready
    ty[5::4, OTHER] = synth.EV_OTHER                     # messages no sensor takes: they count as messages
    t[PAUSE_ROW:, PAUSED] += (1 << 31) + 11              # a pause the 30-bit gap field cannot hold
    ev["types"], ev["times"] = ty, t
    return ev


class Chunked:
    """pekf_frontend_init_resume_dev over row ranges of one resident plane"""

    def __init__(self, eng, planes, form, t_start, n_avg=N_AVG):
        from poseestimationkf_amd import _lib
        self.eng, self.L, self.n_avg = eng, _lib, n_avg
        self.K = planes.shape[1]
        self.flags = eng.EV_F64_EVENTS if form == "f64" else 0
        self.row = planes[0].nbytes
        self.buf = eng.DeviceBuffer(planes.nbytes).upload(planes)
        self.ts = eng.DeviceBuffer(8 * self.K).upload(np.ascontiguousarray(t_start, np.int64))
        nbytes = int(_lib.lib.pekf_frontend_init_state_bytes(self.K, self.flags))
        assert nbytes > 0
        self.state = eng.DeviceBuffer(nbytes)
        self.init, self.t_init = eng.DeviceBuffer(48 * self.K), eng.DeviceBuffer(8 * self.K)
        self.ready = eng.DeviceBuffer(4 * self.K)
        self.started = False

    def _out(self):
        self.L.check(self.L.lib.pekf_device_sync())
        return (self.init.download((self.K, 6), np.float64), self.t_init.download((self.K,), np.int64),
                self.ready.download((self.K,), np.int32).astype(bool))

    def feed(self, a, b):
        self.L.check(self.L.lib.pekf_frontend_init_resume_dev(
            self.K, b - a, self.buf.ptr + a * self.row, self.ts.ptr, self.n_avg, self.init.ptr, self.t_init.ptr,
            self.ready.ptr, self.flags, self.state.ptr, int(self.started), None))
        self.started = True
        return self._out()

    def one_launch(self, n):
        """the existing kernel on the plane's first n rows (stats = NULL), into buffers of its own"""
        p2 = self.eng._launch_phase2(self.K, n, self.buf.ptr, self.ts, self.n_avg, self.flags)
        self.L.check(self.L.lib.pekf_device_sync())
        return (p2.init.download((self.K, 6), np.float64), p2.t_init.download((self.K,), np.int64),
                p2.ready.download((self.K,), np.int32).astype(bool))


def _equal(got, want, label=""):
    assert np.array_equal(got[2], want[2]), label
    assert np.array_equal(got[1], want[1]), label
    assert np.array_equal(np.isnan(got[0]), np.isnan(want[0])), label
    assert np.array_equal(got[0], want[0], equal_nan=True), label


@pytest.fixture(scope="module")
def cases(eng):
    """form -> (stream, packed plane, the one launch on every prefix of its rows): made once, left unchanged"""
    made = {}

    def get(form):
        if form not in made:
            ev = _stream()
            planes = synth.pack_events64(ev, eng.server_event_values(ev)) if form == "f64" else synth.pack_events(ev)
            c = Chunked(eng, planes, form, ev["t_init"])
            made[form] = ev, planes, [c.one_launch(n) for n in range(planes.shape[0] + 1)]
        return made[form]
    return get


def _cuttings(n_rows, prefixes):
    def by(n):
        return [(a, min(a + n, n_rows)) for a in range(0, n_rows, n)]
    rng = np.random.default_rng(7)
    sizes = [0]
    while sum(sizes) < n_rows:
        sizes.append(int(rng.integers(0, 20)))
        if len(sizes) == 2 or rng.random() < 0.3:
            sizes.append(0)
    edges = np.minimum(np.cumsum([0] + sizes + [0]), n_rows)
    cuts = {"1": by(1), "2": by(2), "3": by(3), "7": by(7), "random": list(zip(edges[:-1], edges[1:]))}
    assert sum(a == b for a, b in cuts["random"]) >= 3
    # the number of rows each phone needs to get ready; one gets ready exactly on a chunk's last row, another
    # on a later chunk's first row
    need = np.array([[p[2][k] for p in prefixes].index(True) if prefixes[-1][2][k] else 0 for k in range(K)])
    order = np.argsort(need)
    order = order[need[order] > 0]
    a, b = need[order[0]], need[order[-1]]
    assert 0 < a < b - 1
    cuts["ready at the edges"] = [(0, a), (a, b - 1), (b - 1, n_rows)]
    return cuts


@pytest.mark.parametrize("form", FORMS)
def test_any_cutting_gives_the_one_launch(eng, cases, form):
    ev, planes, prefixes = cases(form)
    n_rows = planes.shape[0]
    whole = eng.frontend_init(ev, n_avg=N_AVG, stats=False, events=form)
    want = (whole["init"], whole["t_init"], whole["ready"])
    _equal(prefixes[-1], want, "the prefix launch on every row")
    assert 0 < want[2].sum() < K                               # not an all-NaN batch, and some never get ready
    assert want[2][OTHER] and want[2][PAUSED]
    if form == "f32":
        assert n_rows == E + 1                                 # the pause became a time event
        te = [r for r in range(n_rows) if synth.has_time_events(planes[r:r + 1, [PAUSED]])]
        assert te == [PAUSE_ROW]
    cuts = _cuttings(n_rows, prefixes)
    if form == "f32":                                          # a time event as a chunk's last row and as a first row
        cuts["time event last"] = [(0, PAUSE_ROW + 1), (PAUSE_ROW + 1, n_rows)]
        cuts["time event first"] = [(0, PAUSE_ROW), (PAUSE_ROW, n_rows)]
    for name, cut in cuts.items():
        c = Chunked(eng, planes, form, ev["t_init"])
        got = None
        for a, b in cut:
            got = c.feed(int(a), int(b))
            _equal(got, prefixes[b], "chunks of %s, after rows %d..%d" % (name, a, b))
        _equal(got, want, "chunks of " + name)


@pytest.mark.parametrize("form", FORMS)
def test_an_empty_first_chunk_starts_the_session(eng, cases, form):
    """n_events == 0 changes nothing but the outputs: with resume == 0 they are the fresh start's"""
    ev, planes, prefixes = cases(form)
    c = Chunked(eng, planes, form, ev["t_init"])
    got = c.feed(0, 0)
    _equal(got, prefixes[0])
    assert not got[2].any() and np.isnan(got[0]).all() and np.array_equal(got[1], ev["t_init"])
    c.feed(0, 9)
    _equal(c.feed(9, 9), prefixes[9])
    _equal(c.feed(9, planes.shape[0]), prefixes[-1])


def test_the_reference_parsers_phase2_trace_in_chunks_of_3(eng):
    """The nine phones of tests/golden/parser.npz, tiled to K columns as tests/test_parser_golden_gpu.py does for
    the one launch, FP64 events fed three rows at a time: ready, t_init and the means the reference's
    InitialValues / Parser ended phase 2 with, bit for bit."""
    z = load_golden()
    phones = [SESSIONS[c % len(SESSIONS)] for c in range(K)]
    streams = [phase_events(z, p, 2) for p in phones]
    ev = _event_dict(streams, np.zeros((K, 3)), np.zeros((K, 3)), [s[2][0] for s in streams])
    planes = synth.pack_events64(ev, eng.server_event_values(ev))
    c = Chunked(eng, planes, "f64", ev["t_init"], n_avg=100)
    n_rows = planes.shape[0]
    for a in range(0, n_rows, 3):
        init, t_init, ready = c.feed(a, min(a + 3, n_rows))
    assert 0 < ready.sum() < K
    for col, p in enumerate(phones):
        assert ready[col] == bool(z[p + "_ready"][0]), (col, p)
        if not ready[col]:
            assert np.isnan(init[col]).all()
            continue
        assert t_init[col] == z[p + "_t_init"][0], (col, p)
        assert same_bits(init[col], np.concatenate([z[p + "_avg"][0], z[p + "_avg"][1]])), (col, p)
