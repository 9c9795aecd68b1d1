"""Wahba operands across pair geometry, weights and scale, for the closed form that replaces Wahba.getRotation's SVD
(Wahba.py:8-17; csrc/pekf_math.hpp make_frame, wahba_rotation, frame_degenerate, wahba_rank1_rotation, behind
k_op<OpWahba>, k_op<OpCorrect>, their n = 1 routes and k_wahba_stream).  NumPy only, deterministic: nothing here comes
from the code under test.  The exact optima and the error of the reference's own float64 statements against them are in
tests/golden/wahba_families.npz (tests/golden/make_wahba_golden.py, mpmath); tests/test_wahba_conditioning_cpu.py pins
both.

An item is (acc0, mag0, acc, mag, k_acc, k_mag).  theta_W is the angle of the reference pair (acc0, mag0), theta_V
that of the current pair (acc, mag), each built as m = cos(theta) a + sin(theta) p with p a unit vector normal to a.
ITEMS = 32 items a family, the kinds of a family taken in turn (item i is of kind i mod the number of kinds):

    ordinary         theta_W, theta_V in U(0.3, 1.3), weights 1/2, 1/2, unit vectors (the other families' defaults)
    thin_current     theta_V in THIN = 1e-2, 1e-4, 1e-6, 1e-8, 1e-10, 3e-12 and pi - 1e-8; theta_W = 1
    thin_reference   the same angles for theta_W; theta_V = 1
    both_thin        theta_W = theta_V in 1e-2, 1e-4
    under_threshold  (theta_V, theta_W) in (5e-13, 1), (1e-13, 1), (1, 5e-13): below the 1e-12 |m| under which
                     frame_degenerate called a pair parallel
    filter_weights   k_acc = |acc_z|, k_mag = 1 - k_acc (ExtendedKalmanFilter.py:71) on unit vectors and on raw units
                     (|acc| = |acc0| = 9.81, |mag| = |mag0| = 48: k_mag < 0 for most), theta_V in 1, 1e-4, 1e-8; theta_W = 1
    lopsided         weights (k, 1 - k), (1 - k, k) and (1 + k, -k) for k in 1e-4, 1e-8, 1e-12
    scale            the current pair times 2^e, e in +-200, +-400, +-520, -540; the reference pair times 2^+-520
    near_optimum     the current pair is the reference pair turned by phi in 1e-2, 1e-4, 1e-6 about a random axis, and
                     by pi - 1e-4 about x, y and z: the optimum is that turn's inverse, near the identity (where
                     RotationMatrix2Quart loses accuracy as 1 / phi) and near each of its three branches' half turn

F32 names the families whose items, rounded to float32, go through the 40 B record (engine.IMUWindow): rounding moves
a thin pair's angle by up to ~1e-7, so only the exact solve of the rounded item says what it is (families32()); a pair
that the rounding makes exactly parallel (exactly_parallel()) has rank 1 and is judged as the groups below.

Judged apart, by the optimum tr(R^T B) (tests/test_degenerate_samples.py), not against an exact rotation:

    rank1_by_weight()   k_acc = 0 exactly and k_mag = 0 exactly, ordinary frames: B = w v^T from healthy pairs
    parallels()         mag = s acc (the current pair, even items) or mag0 = s acc0 (odd items) for PARALLELS = 1000
                        random acc and s, then test_degenerate_samples' CASES: these must take the rank-1 route
                        (parallels32(): the current-pair ones in float32 values, for the 40 B record)
    overflow()          both pairs times 2^520: B is not finite, the reference raises "SVD did not converge"
"""
import numpy as np

SEED = 20261021
ITEMS = 32
PARALLELS = 1000
MARGIN = 8.0                      # a device solve over the reference's own statement (tests/percall_families.py)
U = 2.0 ** -53                    # the IEEE routes' unit roundoff
RSQRT = 4.2e-15                   # the FAST route's rsqrt bound (19 ulp, pekf_math.hpp, scripts/probe_fp64.hip)
FAST_MARGIN = MARGIN * RSQRT / U  # ~ 303
INFORMATIVE = 0.5                 # a wrong rotation's error is O(1): a family is asserted only below this bound
SIGN_MARGIN = 1e-3
FIELDS = ("acc0", "mag0", "acc", "mag", "k_acc", "k_mag")

THIN = (1e-2, 1e-4, 1e-6, 1e-8, 1e-10, 3e-12, np.pi - 1e-8)
UNDER = ((5e-13, 1.0), (1e-13, 1.0), (1.0, 5e-13))          # (theta_V, theta_W)
LOPSIDED_K = (1e-4, 1e-8, 1e-12)
SCALE = tuple(("current", e) for e in (200, -200, 400, -400, 520, -520, -540)) + (("reference", 520), ("reference", -520))
PHI = (1e-2, 1e-4, 1e-6)
NAMES = ["ordinary", "thin_current", "thin_reference", "both_thin", "under_threshold", "filter_weights", "lopsided",
         "scale", "near_optimum"]
F32 = ["ordinary", "thin_current", "thin_reference", "both_thin", "lopsided", "near_optimum"]
STREAM = [n for n in NAMES if n != "scale"]     # k_wahba_stream is no drop-in: no promise far from unit scale


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _normal_to(rng, a):
    p = np.cross(a, _unit(rng, len(a)))
    return p / np.linalg.norm(p, axis=1, keepdims=True)


def pair(rng, theta):
    """unit a, and m = cos(theta) a + sin(theta) p, for each angle of theta"""
    theta = np.asarray(theta, dtype=np.float64)
    a = _unit(rng, len(theta))
    p = _normal_to(rng, a)
    return a, np.cos(theta)[:, None] * a + np.sin(theta)[:, None] * p


def _items(rng, theta_w, theta_v, ka=0.5, km=0.5):
    acc0, mag0 = pair(rng, theta_w)
    acc, mag = pair(rng, theta_v)
    return dict(acc0=acc0, mag0=mag0, acc=acc, mag=mag, k_acc=np.full(ITEMS, ka), k_mag=np.full(ITEMS, km))


def _turn(i):
    return np.arange(ITEMS) % i


def rodrigues(axis, phi):
    k = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3) + np.sin(phi) * k + (1.0 - np.cos(phi)) * (k @ k)


def kinds(name):
    """the kind of each item of a family, as a label"""
    if name in ("thin_current", "thin_reference"):
        return ["%.0e" % THIN[i] if i < 6 else "pi-1e-8" for i in _turn(7)]
    if name == "both_thin":
        return ["1e-02", "1e-04"] * (ITEMS // 2)
    if name == "under_threshold":
        return ["V %.0e" % UNDER[i][0] if UNDER[i][1] == 1.0 else "W %.0e" % UNDER[i][1] for i in _turn(3)]
    if name == "filter_weights":
        return ["%s %.0e" % ("unit" if i < 3 else "raw", (1.0, 1e-4, 1e-8)[i % 3]) for i in _turn(6)]
    if name == "lopsided":
        return ["%s %.0e" % (("k,1-k", "1-k,k", "1+k,-k")[i // 3], LOPSIDED_K[i % 3]) for i in _turn(9)]
    if name == "scale":
        return ["%s %+d" % SCALE[i] for i in _turn(9)]
    if name == "near_optimum":
        return ["%.0e" % PHI[i] if i < 3 else "pi-1e-4 " + "xyz"[i - 3] for i in _turn(6)]
    return ["ordinary"] * ITEMS


def stream_pick(name):
    """The items of a family that k_wahba_stream (the FAST route) is held to: under today's threshold only 5e-13,
    where its bound is still informative; Y is then taken over these items alone"""
    return np.array([name != "under_threshold" or not k.endswith("1e-13") for k in kinds(name)])


def _family(name, rng):
    ordinary = lambda: rng.uniform(0.3, 1.3, ITEMS)
    one = np.ones(ITEMS)
    if name == "ordinary":
        return _items(rng, ordinary(), ordinary())
    if name == "thin_current":
        return _items(rng, one, np.array(THIN)[_turn(7)])
    if name == "thin_reference":
        return _items(rng, np.array(THIN)[_turn(7)], one)
    if name == "both_thin":
        th = np.array([1e-2, 1e-4])[_turn(2)]
        return _items(rng, th, th)
    if name == "under_threshold":
        u = np.array(UNDER)[_turn(3)]
        return _items(rng, u[:, 1], u[:, 0])
    if name == "filter_weights":
        f = _items(rng, one, np.array([1.0, 1e-4, 1e-8])[_turn(3)])
        raw = _turn(6) >= 3
        for k, s in (("acc0", 9.81), ("acc", 9.81), ("mag0", 48.0), ("mag", 48.0)):
            f[k] = np.where(raw[:, None], s * f[k], f[k])
        f["k_acc"] = np.abs(f["acc"][:, 2])
        f["k_mag"] = 1.0 - f["k_acc"]
        return f
    if name == "lopsided":
        f = _items(rng, ordinary(), ordinary())
        k = np.array(LOPSIDED_K)[_turn(9) % 3]
        form = _turn(9) // 3
        f["k_acc"] = np.where(form == 0, k, np.where(form == 1, 1.0 - k, 1.0 + k))
        f["k_mag"] = np.where(form == 0, 1.0 - k, np.where(form == 1, k, -k))
        return f
    if name == "scale":
        f = _items(rng, ordinary(), ordinary())
        for i, j in enumerate(_turn(9)):
            which, e = SCALE[j]
            for k in (("acc", "mag") if which == "current" else ("acc0", "mag0")):
                f[k][i] = np.ldexp(f[k][i], e)
        return f
    if name == "near_optimum":
        f = _items(rng, ordinary(), one)
        axes = _unit(rng, ITEMS)
        for i, j in enumerate(_turn(6)):
            T = rodrigues(axes[i], PHI[j]) if j < 3 else rodrigues(np.eye(3)[j - 3], np.pi - 1e-4)
            f["acc"][i], f["mag"][i] = T @ f["acc0"][i], T @ f["mag0"][i]
        return f
    raise KeyError(name)


_cache = {}


def families():
    """{name: {field: (ITEMS, ..) float64}} in NAMES' order (read-only, built once)"""
    if "f64" not in _cache:
        out = {n: _family(n, np.random.default_rng([SEED, 7, i])) for i, n in enumerate(NAMES)}
        for f in out.values():
            for a in f.values():
                a.setflags(write=False)
        _cache["f64"] = out
    return _cache["f64"]


def families32():
    """The F32 families with every vector rounded to float32 (held as float64): what the 40 B record can carry"""
    if "f32" not in _cache:
        out = {}
        for n in F32:
            f = {k: (v.astype(np.float32).astype(np.float64) if v.ndim == 2 else v.copy()) for k, v in families()[n].items()}
            for a in f.values():
                a.setflags(write=False)
            out[n] = f
        _cache["f32"] = out
    return _cache["f32"]


def pair_parallel(a, m):
    """a x m = 0 exactly (each product compared exactly, which float32 values held as float64 allow; a zero vector
    counts).  False for every item unless all entries are float32 values."""
    with np.errstate(over="ignore"):
        if not all(np.array_equal(x.astype(np.float32).astype(np.float64), x) for x in (a, m)):
            return np.zeros(len(a), bool)
    return ((a[:, 1] * m[:, 2] == a[:, 2] * m[:, 1]) & (a[:, 2] * m[:, 0] == a[:, 0] * m[:, 2])
            & (a[:, 0] * m[:, 1] == a[:, 1] * m[:, 0]))


def exactly_parallel(f):
    """Items one of whose pairs is exactly parallel"""
    return pair_parallel(f["acc"], f["mag"]) | pair_parallel(f["acc0"], f["mag0"])


def side_by_side(fam, names=None):
    """The families' operands in one batch, and {name: slice} of its rows"""
    names = list(fam) if names is None else names
    cat = {k: np.concatenate([fam[n][k] for n in names]) for k in FIELDS}
    return cat, {n: slice(i * ITEMS, (i + 1) * ITEMS) for i, n in enumerate(names)}


def matrices():
    """{name: (ITEMS, 3, 3)} for the pure R -> q operator (RotationMatrix2Quart, Wahba.py:19-47), the float64 matrices as
    given: turns by phi in PHI about random axes (all three branches lose accuracy as 1 / phi), and by pi - 1e-4 about x,
    y, z and axes within 1e-3 of them (a half turn's branch: w's numerator is ~2e-4)"""
    if "mat" not in _cache:
        rng = np.random.default_rng([SEED, 8])
        axes = _unit(rng, ITEMS)
        near = np.stack([rodrigues(axes[i], PHI[i % 3]) for i in range(ITEMS)])
        half = np.empty((ITEMS, 3, 3))
        for i in range(ITEMS):
            ax = np.eye(3)[i % 3] + (1e-3 * axes[i] if i >= 3 else 0.0)
            half[i] = rodrigues(ax / np.linalg.norm(ax), np.pi - 1e-4)
        near.setflags(write=False)
        half.setflags(write=False)
        _cache["mat"] = {"near_identity": near, "near_half_turn": half}
    return _cache["mat"]


# ------------------------------------------------------------------------------------------ judged by the optimum
ACC0, MAG0 = np.array([0.0, 0.1, 0.99]), np.array([0.5, 0.0, -0.86])
CASES = {   # tests/test_degenerate_samples.py's: (acc, mag) of the current sample, (acc0, mag0) of the reference pair
    "zero acc": ([0.0, 0.0, 0.0], [0.45, 0.05, -0.88], ACC0, MAG0),
    "zero mag": ([0.02, 0.1, 0.98], [0.0, 0.0, 0.0], ACC0, MAG0),
    "acc parallel to mag": ([0.1, -0.2, 0.95], [0.2, -0.4, 1.9], ACC0, MAG0),
    "reference pair parallel": ([0.02, 0.1, 0.98], [0.45, 0.05, -0.88], ACC0, 2.0 * ACC0),
}


def rank1_by_weight():
    """16 ordinary items, k_acc = 0 exactly on the even ones and k_mag = 0 exactly on the odd ones (the other weight 1)"""
    rng = np.random.default_rng([SEED, 9])
    n = 16
    acc0, mag0 = pair(rng, rng.uniform(0.3, 1.3, n))
    acc, mag = pair(rng, rng.uniform(0.3, 1.3, n))
    even = np.arange(n) % 2 == 0
    return dict(acc0=acc0, mag0=mag0, acc=acc, mag=mag, k_acc=np.where(even, 0.0, 1.0), k_mag=np.where(even, 1.0, 0.0))


def parallels():
    """PARALLELS items with one pair parallel as float64 products give it (mag = s acc, each entry rounded once; s of
    either sign, |s| in 1/8 .. 8, |acc| in 1/4 .. 16), the current pair on even items and the reference pair on odd
    ones, weights 1/2, 1/2; then CASES with the filter's weights.  `current` marks the items whose reference pair is
    healthy (the ones k_wahba_stream and the fused kernels' rank-1 route serve)."""
    rng = np.random.default_rng([SEED, 10])
    n = PARALLELS
    f = dict(zip(("acc0", "mag0"), pair(rng, rng.uniform(0.3, 1.3, n))))
    f.update(zip(("acc", "mag"), pair(rng, rng.uniform(0.3, 1.3, n))))
    a = _unit(rng, n) * np.exp2(rng.uniform(-2.0, 4.0, n))[:, None]
    s = (np.exp2(rng.uniform(-3.0, 3.0, n)) * rng.choice([-1.0, 1.0], n))[:, None]
    even = (np.arange(n) % 2 == 0)[:, None]
    f["acc"], f["mag"] = np.where(even, a, f["acc"]), np.where(even, s * a, f["mag"])
    f["acc0"], f["mag0"] = np.where(even, f["acc0"], a), np.where(even, f["mag0"], s * a)
    f["k_acc"], f["k_mag"] = np.full(n, 0.5), np.full(n, 0.5)
    c = {k: np.array([np.asarray(v[i], dtype=np.float64) for v in CASES.values()]) for i, k in ((2, "acc0"), (3, "mag0"), (0, "acc"), (1, "mag"))}
    c["k_acc"] = np.abs(c["acc"][:, 2])
    c["k_mag"] = 1.0 - c["k_acc"]
    out = {k: np.concatenate([f[k], c[k]]) for k in FIELDS}
    out["current"] = np.concatenate([even[:, 0], [True, True, True, False]])
    return out


def parallels32():
    """parallels()' current-pair items for the 40 B record: acc rounded to float32 and mag = +-2^j acc, j in -3 .. 3, so
    that the pair is exactly parallel in float32 too; the reference pair rounded to float32; weights 1/2, 1/2"""
    rng = np.random.default_rng([SEED, 12])
    p = parallels()
    pick = p["current"][:PARALLELS]
    r32 = lambda v: v.astype(np.float32).astype(np.float64)
    f = {k: r32(p[k][:PARALLELS][pick]) for k in ("acc0", "mag0", "acc")}
    n = len(f["acc"])
    f["mag"] = np.ldexp(f["acc"], rng.integers(-3, 4, n)[:, None]) * rng.choice([-1.0, 1.0], n)[:, None]
    f["k_acc"], f["k_mag"] = np.full(n, 0.5), np.full(n, 0.5)
    return f


def overflow():
    """4 ordinary items, both pairs times 2^520: every entry of B overflows"""
    rng = np.random.default_rng([SEED, 11])
    n = 4
    acc0, mag0 = pair(rng, rng.uniform(0.3, 1.3, n))
    acc, mag = pair(rng, rng.uniform(0.3, 1.3, n))
    return dict(acc0=np.ldexp(acc0, 520), mag0=np.ldexp(mag0, 520), acc=np.ldexp(acc, 520), mag=np.ldexp(mag, 520),
                k_acc=np.full(n, 0.5), k_mag=np.full(n, 0.5))


def stacked():
    """Every finite-B item in one batch: the NAMES families side by side, then rank1_by_weight and parallels; and
    {name: slice} of its rows"""
    fam = families()
    cat, sl = side_by_side(fam, NAMES)
    at = len(cat["acc"])
    for name, f in (("rank1_by_weight", rank1_by_weight()), ("parallels", parallels())):
        cat = {k: np.concatenate([cat[k], f[k]]) for k in FIELDS}
        sl[name] = slice(at, at + len(f["acc"]))
        at += len(f["acc"])
    return cat, sl


# ------------------------------------------------------------------------------------------ judging
def golden():
    """tests/golden/wahba_families.npz (make_wahba_golden.py says what it holds), read once"""
    if "golden" not in _cache:
        import os
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wahba_families.npz")) as z:
            _cache["golden"] = {k: z[k] for k in z.files}
    return _cache["golden"]


def yard(g, which, rows, pick=None):
    """(Y_R, Y_q) of the items rows (a slice) of set which ("f64", "f32"), those of pick (bool over the slice) if given:
    the worst error of the reference's own float64 statement, exactly parallel items left out"""
    eR, eq = g[which + "_err_R"][rows], g[which + "_err_q"][rows]
    if pick is not None:
        eR, eq = eR[pick], eq[pick]
    return float(np.nanmax(eR)), float(np.nanmax(eq))


def sign_qualifies(g, which):
    """Items whose q must carry the reference's sign: the exact branch margin above SIGN_MARGIN of the chosen numerator
    (near the identity all three numerators are of order phi^2, and the choice is as safe as the margin is beside them;
    taken absolutely the margin would leave out a whole family and a ninth of the items with it) and w's exact
    numerator above SIGN_MARGIN."""
    with np.errstate(invalid="ignore"):
        return (g[which + "_margin"] > SIGN_MARGIN * g[which + "_t_own"]) & (g[which + "_w_num"] > SIGN_MARGIN)


def wahba_b(f, i=None):
    """B of the reference (Wahba.py:11-13), of item i or of every item"""
    if i is not None:
        return f["k_acc"][i] * np.outer(f["acc0"][i], f["acc"][i]) + f["k_mag"][i] * np.outer(f["mag0"][i], f["mag"][i])
    return (f["k_acc"][:, None, None] * (f["acc0"][:, :, None] * f["acc"][:, None, :])
            + f["k_mag"][:, None, None] * (f["mag0"][:, :, None] * f["mag"][:, None, :]))


def err_rotation(R, R_exact):
    """max |R - R_exact| per item; inf where R is not finite"""
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    with np.errstate(invalid="ignore"):
        e = np.abs(R - R_exact).max(axis=(1, 2))
    return np.where(np.isfinite(R).all(axis=(1, 2)), e, np.inf)


def err_quat(q, q_exact):
    """min(max |q - q_exact|, max |q + q_exact|) per item; inf where q is not finite"""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        e = np.minimum(np.abs(q - q_exact).max(axis=1), np.abs(q + q_exact).max(axis=1))
    return np.where(np.isfinite(q).all(axis=1), e, np.inf)


def same_sign(q, q_ref):
    """q is nearer q_ref than -q_ref, per item"""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
    return np.abs(q - q_ref).max(axis=1) <= np.abs(q + q_ref).max(axis=1)


def quat_rotm(q):
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
    w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=-1).reshape(-1, 3, 3)


def optimum_shortfall(R, f):
    """Per item: how far R is from proper orthogonal (max |R R^T - I|, |det R - 1|) and how far tr(R^T B) falls short
    of the optimum sigma_1 + sigma_2 of B (NumPy's singular values; sigma_3 = 0 for two pairs), as a share of sigma_1."""
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    B = wahba_b(f)
    sv = np.linalg.svd(B, compute_uv=False)
    orth = np.maximum(np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max(axis=(1, 2)), np.abs(np.linalg.det(R) - 1.0))
    short = (sv[:, 0] + sv[:, 1] - np.einsum("nij,nij->n", R, B)) / sv[:, 0]
    return orth, short
