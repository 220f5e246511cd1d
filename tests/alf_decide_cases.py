"""What EncAdaptiveLoopFilter::alfEncoder reads of the per-CTU covariance records, restated for the tests of vvcgpu_alf_frame_stats and
vvcgpu_alf_ctu_dist: getFrameStat (EncAdaptiveLoopFilter.cpp:1303-1315) as an int64 sum, and the two per-CTU distortions of deriveCtbAlfEnableFlags
(getUnfilteredDistortion :618-626, getFilteredDistortion :628-639 with calcErrorForCoeffs :1157-1174) in numpy float64 -- IEEE doubles as the x86
reference's -- one operation at a time in the reference's order (vectorised over the CTUs only, which changes no operation).  The same function
evaluates three WRONG orders, which the fixture uses to prove that its large-magnitude records tell the orders apart.  tests/golden/alf_decide.npz
pins all of it to the compiled reference (tests/test_alf_decide_cpu.py).  Also the seeded record generators that the fixture generator, the tests and
tools/alf_decide_time.py share: the fixture stores seeds and parameters, never records.  numpy only."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "alf_decide.npz")
N_OF = {0: 7, 1: 13}                     # filter_type -> coefficients of the shape
REAL, NOISE, LARGE = 0, 1, 2             # record sets
ORDERS = ("reference", "classes_reversed", "class_tree", "row_tree")
LARGE_SHIFT = {13: 20, 7: 22}            # the large set: Gram records << shift plus `shift` bits of independent noise, 46 to 48 bits (the short rows
                                         # of the 5x5 shape need the larger values for their sums to pass 2^53)


def n_vals(N):
    return N * N + N + 1


def split(rec, N):
    """records (..., N*N+N+1) -> E (..., N, N), y (..., N), pixAcc (...)"""
    return rec[..., :N * N].reshape(rec.shape[:-1] + (N, N)), rec[..., N * N:N * N + N], rec[..., N * N + N]


def pack(E, y, pix):
    return np.ascontiguousarray(np.concatenate([E.reshape(E.shape[:-2] + (-1,)), y, pix[..., None]], axis=-1).astype(np.int64))


# ---- record sets ---------------------------------------------------------------------------------------------------------------------------------
def real_records(filter_type):
    """the compiled reference's records of the 136x72 picture c0 of alf.npz: 6 CTUs x 25 classes (some classes empty)"""
    return np.ascontiguousarray(np.load(os.path.join(HERE, "golden", "alf.npz"))["c0_stats_f%d" % filter_type])


def _gram(X, d):
    """E = X'X, y = X'd, pixAcc = d'd per (CTU, class)"""
    return pack(np.einsum("abki,abkj->abij", X, X), np.einsum("abki,abk->abi", X, d), (d * d).sum(-1))


def noise_records(seed, n_ctu, n_cls, N, samples=24):
    """Gram matrices of sample vectors: per (CTU, class) `samples` positions with N neighbour sums of two 10-bit samples each and an error
    org - rec in -64..64, independent of them (y of either sign)"""
    rng = np.random.default_rng([seed, n_ctu, n_cls, N])
    X = rng.integers(0, 2047, (n_ctu, n_cls, samples, N), dtype=np.int64)
    d = rng.integers(-64, 65, (n_ctu, n_cls, samples), dtype=np.int64)
    return _gram(X, d)


def large_records(seed, n_ctu, n_cls, N, n_filters, coeff_bits, samples=24):
    """Records on which a summation order shows.  Two things make it show.  Magnitude: Gram records shifted up by LARGE_SHIFT bits, the freed low bits
    filled with independent noise (symmetric in E) -- 46-bit values whose products and sums no longer fit 53 bits.  Cancellation: the error org - rec
    of a position is noise plus a multiple of what the class's own filter (coeff_set / filter_indices of the same seed) predicts.  Half the
    prediction in the middle classes: c'Ec / factor and 2 c'y nearly cancel, the roundings of the row sums reach the leading bits of a small class
    result.  None in the first class and the whole prediction in the last, which share samples and filter: results +Q and nearly -Q, so the running
    sum over the classes is large (coarse roundings) while the CTU's result is small (they show)."""
    shift = LARGE_SHIFT[N]
    rng = np.random.default_rng([seed, n_ctu, n_cls, N, shift])
    X = rng.integers(0, 2047, (n_ctu, n_cls, samples, N), dtype=np.int64)
    X[:, -1] = X[:, 0]
    c = coeff_set(seed, n_filters, N)[filter_indices(seed, n_cls, n_filters)].astype(np.int64)
    halves = np.array([1] if n_cls == 1 else [0] + [1] * (n_cls - 2) + [2], np.int64)
    d = np.einsum("abki,bi->abk", X, c * halves[:, None]) // (1 << coeff_bits) + rng.integers(-64, 65, (n_ctu, n_cls, samples), dtype=np.int64)
    E, y, pix = split(_gram(X, d), N)
    lo = rng.integers(0, 1 << shift, E.shape, dtype=np.int64)
    lo = np.triu(lo) + np.swapaxes(np.triu(lo, 1), -1, -2)
    rec = pack((E << shift) + lo, (y << shift) + rng.integers(0, 1 << shift, y.shape, dtype=np.int64),
               (pix << shift) + rng.integers(0, 1 << shift, pix.shape, dtype=np.int64))
    assert int(np.abs(rec).max()) < 1 << 53
    return rec


def records(kind, seed, n_ctu, n_cls, filter_type, n_filters=1, coeff_bits=10):
    """the records of one case; n_filters and coeff_bits matter to the large set only"""
    N = N_OF[filter_type]
    if kind == REAL:
        rec = real_records(filter_type)
        reps = -(-n_ctu // rec.shape[0])
        return np.ascontiguousarray(np.concatenate([rec] * reps)[:n_ctu, :n_cls])
    if kind == NOISE:
        return noise_records(seed, n_ctu, n_cls, N)
    return large_records(seed, n_ctu, n_cls, N, n_filters, coeff_bits)


def coeff_set(seed, n_filters, N, amp=60):
    """quantised filters as the encoder's: small taps, the centre tap completing the DC gain 512 (= 1.0 at 10 bits)"""
    rng = np.random.default_rng([seed, n_filters, N, 77])
    c = rng.integers(-amp, amp + 1, (n_filters, N)).astype(np.int32)
    c[:, N - 1] = 512 - 2 * c[:, :N - 1].sum(1)
    return c


def filter_indices(seed, n_cls, n_filters):
    """every filter in use where the classes suffice (with 25 filters all but one); the first and the last class share theirs, and with fewer
    filters than classes so do others"""
    rng = np.random.default_rng([seed, n_cls, n_filters, 78])
    idx = rng.integers(0, n_filters, n_cls).astype(np.int16)
    idx[:min(n_cls, n_filters)] = np.arange(min(n_cls, n_filters))
    idx = rng.permutation(idx).astype(np.int16)
    if n_cls > 1:
        others = [f for f in range(n_filters) if f not in idx[:-1]]
        idx[-1] = idx[0]
        if others and n_cls > 2:
            idx[1] = others[0]           # the filter the last class gave up
    return idx


def enable_mask(seed, n_ctu, mode):
    """mode 'on' | 'off' | 'mixed'"""
    if mode != "mixed":
        return np.full(n_ctu, 1 if mode == "on" else 0, np.uint8)
    m = np.random.default_rng([seed, n_ctu, 79]).integers(0, 2, n_ctu).astype(np.uint8)
    if n_ctu > 1:
        m[0], m[-1] = 1, 0
    return m


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------------
def frame_stats(rec, enable=None):
    """getFrameStat into a reset frame record: int64 (n_classes, n_vals)"""
    on = np.ones(rec.shape[0], bool) if enable is None else np.asarray(enable) != 0
    return rec[on].sum(0, dtype=np.int64)


def _tree(xs):
    xs = list(xs)
    while len(xs) > 1:
        xs = [xs[k] + xs[k + 1] if k + 1 < len(xs) else xs[k] for k in range(0, len(xs), 2)]
    return xs[0]


def _chain(xs, zero):
    s = zero
    for x in xs:
        s = s + x
    return s


def class_error(E, y, coeff, coeff_bits, row_tree=False):
    """calcErrorForCoeffs for every CTU at once: E (n, N, N), y (n, N) float64, coeff N ints"""
    N = len(coeff)
    factor = np.float64(1 << (coeff_bits - 1))
    c = [np.float64(int(v)) for v in coeff]
    zero = np.zeros(E.shape[0], np.float64)
    error = zero
    for i in range(N):
        prods = [E[:, i, j] * c[j] for j in range(i + 1, N)]
        s = _tree(prods) if row_tree and prods else _chain(prods, zero)
        error = error + ((E[:, i, i] * c[i] + s * np.float64(2)) / factor - np.float64(2) * y[:, i]) * c[i]
    return error / factor


def ctu_dist(rec, coeffs, filter_idx, coeff_bits=10, order="reference"):
    """-> float64 (n_ctu, 2): [:, 0] getUnfilteredDistortion(cov, numClasses), [:, 1] getFilteredDistortion.  `order` other than "reference" is a
    deliberately wrong summation order (ORDERS), for the fixture's proof only"""
    assert order in ORDERS
    n, n_cls, nv = rec.shape
    N = 13 if nv == 183 else 7
    assert nv == n_vals(N)
    coeffs = np.asarray(coeffs).reshape(-1, N)
    idx = np.zeros(n_cls, np.int64) if filter_idx is None else np.asarray(filter_idx, np.int64)
    E, y, pix = (a.astype(np.float64) for a in split(rec, N))           # exact below 2^53
    zero = np.zeros(n, np.float64)
    with np.errstate(all="raise"):
        errs = [class_error(E[:, k], y[:, k], coeffs[idx[k]], coeff_bits, order == "row_tree") for k in range(n_cls)]
        if order == "classes_reversed":
            errs = errs[::-1]
        filt = _tree(errs) if order == "class_tree" else _chain(errs, zero)
        unf = _chain([pix[:, k] for k in range(n_cls)], zero)
    return np.ascontiguousarray(np.stack([unf, filt], axis=1))


def bits(a):
    """doubles as their 64-bit patterns"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------------
META = ("kind", "seed", "n_ctu", "n_cls", "filter_type", "n_filters", "coeff_bits")


def load_golden():
    """-> list of cases: dict of the META ints, 'coeff', 'idx', 'enable', and the reference's 'frame' (int64) and 'dist' (float64)"""
    g = np.load(GOLDEN)
    out = []
    for i in range(int(g["n_cases"])):
        k = "k%d_" % i
        c = dict(zip(META, (int(v) for v in g[k + "meta"])))
        c.update(coeff=g[k + "coeff"], idx=g[k + "idx"], enable=g[k + "enable"], frame=g[k + "frame"], dist=g[k + "dist"], id="k%d" % i)
        out.append(c)
    return out


def case_records(c):
    return records(*(c[m] for m in META))


def check_fixture(cases, wrong_orders):
    """the properties the tests rely on; wrong_orders(case) -> {order: float64 (n_ctu, 2)} for the cases of the large set"""
    facts = set()
    for c in cases:
        N = N_OF[c["filter_type"]]
        rec = case_records(c)
        facts.add(("shape", c["filter_type"]))
        facts.add(("classes", c["n_cls"]))
        facts.add(("bits", c["coeff_bits"] == 10))
        if c["n_cls"] == 25 and len(set(c["idx"].tolist())) < 25 and c["n_filters"] > 1:
            facts.add("shared_filter")
        if (c["coeff"] == 0).all(1).any() and (c["coeff"][c["idx"]] == 0).all(1).any():
            facts.add("zero_filter_in_use")
        if (split(rec, N)[1] < 0).any():
            facts.add("negative_y")
        facts.add(("mask", "on" if c["enable"].all() else "off" if not c["enable"].any() else "mixed"))
        if c["kind"] == LARGE:
            ref = bits(c["dist"])[:, 1]
            for order, d in wrong_orders(c).items():
                changed = int((bits(d)[:, 1] != ref).sum())
                assert 4 * changed >= c["n_ctu"], "large set %s: order '%s' changes only %d of %d CTUs" % (c["id"], order, changed, c["n_ctu"])
                facts.add(("order_visible", order, c["n_cls"] > 1 or order == "row_tree"))
    want = [("shape", 0), ("shape", 1), ("classes", 25), ("classes", 1), ("bits", True), ("bits", False), "shared_filter", "zero_filter_in_use",
            "negative_y", ("mask", "on"), ("mask", "off"), ("mask", "mixed")] + [("order_visible", o, True) for o in ORDERS[1:]]
    for f in want:
        assert f in facts, (f, sorted(map(str, facts)))


def wrong_orders_restated(c):
    rec = case_records(c)
    orders = ORDERS[1:] if c["n_cls"] > 1 else ("row_tree",)          # one class: the class orders are all the same
    return {o: ctu_dist(rec, c["coeff"], c["idx"], c["coeff_bits"], o) for o in orders}
