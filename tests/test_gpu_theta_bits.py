"""Decisions per entry of Theta = W^T H leaving the device as bits: nbmf_theta_bits (Context.theta_bits) in its two modes,
"theta > threshold" and the Bernoulli draw "u < theta", and the estimator methods on top (predict(packed=True), sample).

YARDSTICKS.  Everything is compared EXACTLY, against code that existed before this path did: Context.predict_rows (the
device's own float64 Theta and its thresholded bytes), NumPy (packbits, the comparison) and _hip.synthetic_reference /
_hip.hash_uniform (the NumPy regeneration of the device's counter-based uniform).  The kernel opens with the same tile as
predict_rows_kernel, so its Theta is bit for bit the one predict_rows returns: no tolerance enters anywhere.

CASES.  The factors of tests/test_gpu_predict.py::case: default_rng(1000 + k), W k x m uniform(0.1, 0.9) with columns
normalised, H k x n uniform(0.1, 0.9).  37 x 53 for k in 1, 3, 4, 5, 16, 17, 40, 130; 130 x 257 at k = 5 and 40 (several
64-column strips, two workgroups of columns, the 128 padding crossed both ways); 17 x n for n in 1, 8, 63, 64, 65 at k = 5:
a lone pad-filled byte, one whole byte, the last bit of a strip missing, exactly one strip, one bit into the next.

STATISTICS (test 3).  At 256 x 512 and density 0.3 an entry's variance is 0.21, so sigma of the overall mean is
sqrt(0.21 / 131072), of a row mean sqrt(0.21 / 512) and of a column mean sqrt(0.21 / 256); the bound is 5 sigma each.  Checked on
the CPU with synthetic_reference for all five seeds before the assertion was written: the overall means lie within 1.7
sigma, every row mean within 3.4 and every column mean within 3.9."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = (1, 3, 4, 5, 16, 17, 40, 130)
WIDE = ((5, 130, 257), (40, 130, 257))
NARROW = tuple((5, 17, n) for n in (1, 8, 63, 64, 65))
SHAPES = tuple((k, 37, 53) for k in KS) + WIDE + NARROW
SEEDS = (0, 1, 2 ** 63 + 5, 2 ** 64 - 1)
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def hip():
    from nbmf_mm_amd import _hip
    assert _hip.device_count() >= 1, "no MI355X visible: the GPU tests must run on the GPU box"
    return _hip


_cases = {}


def case(k, m=37, n=53):
    """(W k x m, H k x n) of case k, as tests/test_gpu_predict.py::case draws them; made once and shared (read-only)."""
    key = (k, m, n)
    if key not in _cases:
        r = np.random.default_rng(1000 + k)
        W = r.uniform(0.1, 0.9, (k, m))
        W /= W.sum(0)
        H = r.uniform(0.1, 0.9, (k, n))
        for a in (W, H):
            a.setflags(write=False)
        _cases[key] = (W, H)
    return _cases[key]


def context(hip, W, H):
    ctx = hip.Context(W.shape[1], H.shape[1], W.shape[0])
    ctx.set_factors(W, H)
    return ctx


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def packed(dense):
    return np.packbits(dense, axis=1)


# ---- 1. threshold mode: the bits of the byte path ------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m,n", SHAPES)
def test_threshold_bits_are_the_packed_bytes_of_predict_rows(hip, k, m, n):
    from nbmf_mm_amd import PackedBits
    W, H = case(k, m, n)
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        i_eq, j_eq = m // 2, n // 2
        t_eq = float(theta[i_eq, j_eq])
        for t in (-1.0, 0.0, 0.5, 1.0, 2.0, float(np.median(theta)), t_eq):
            got = ctx.theta_bits(threshold=t)
            assert isinstance(got, PackedBits) and got.shape == (m, n)
            assert got.bits.dtype == np.uint8 and got.bits.shape == (m, (n + 7) // 8)
            want = ctx.predict_rows(threshold=t)
            assert np.array_equal(got.bits, packed(want)), f"threshold {t!r}"        # (byte for byte: the pad bits are zeros)
        eq = ctx.theta_bits(threshold=t_eq).toarray()
        assert not eq[i_eq, j_eq], "theta > threshold must be strict"
        assert np.array_equal(eq, theta > t_eq)
        assert ctx.theta_bits(threshold=-1.0).toarray().all() and not ctx.theta_bits(threshold=2.0).bits.any()


# ---- 2. sample mode: u < theta with the device's own theta -----------------------------------------------------------------
@pytest.mark.parametrize("k,m,n", SHAPES)
def test_sample_bits_are_hash_uniform_below_theta(hip, k, m, n):
    W, H = case(k, m, n)
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        draws = []
        for s in SEEDS:
            got = ctx.theta_bits(seed=s)
            want = hip.hash_uniform(m, n, s) < theta
            assert np.array_equal(got.toarray(), want), f"seed {s}"
            assert np.array_equal(got.bits, packed(want)), f"seed {s}: pad bits"
            assert np.array_equal(got.bits, ctx.theta_bits(seed=s).bits), f"seed {s}: the same call twice"
            draws.append(got.bits)
        if m * n >= 64:                                       # (17 x 1 and 17 x 8 may well agree by chance)
            for a in range(len(SEEDS)):
                for b in range(a):
                    assert not np.array_equal(draws[a], draws[b])


# ---- 3. the tie to the existing generator -------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", ((37, 53), (256, 512)))
@pytest.mark.parametrize("d", (0.25, 0.3))
def test_constant_theta_reproduces_the_synthetic_generator(hip, m, n, d):
    """k = 1, W = 1, H = d: Theta = 1 * d = d exactly, and the draw is ``u < d``: what Context.generate plants."""
    W, H = np.ones((1, m)), np.full((1, n), d)
    with context(hip, W, H) as ctx:
        assert np.all(ctx.predict_rows() == d)
        for s in (0, 1, 7, 2 ** 63 + 5, 2 ** 64 - 1):
            got = ctx.theta_bits(seed=s).toarray()
            assert np.array_equal(got, hip.synthetic_reference(m, n, s, density=d)[0] != 0), f"seed {s}"
            if (m, n, d) == (256, 512, 0.3):
                var = d * (1 - d)
                z = (got.mean() - d) / np.sqrt(var / (m * n))
                zr = np.abs(got.mean(axis=1) - d).max() / np.sqrt(var / n)
                zc = np.abs(got.mean(axis=0) - d).max() / np.sqrt(var / m)
                print(f"seed {s}: mean {z:+.2f} sigma, worst row {zr:.2f} sigma, worst column {zc:.2f} sigma")
                assert abs(z) <= 5 and zr <= 5 and zc <= 5


# ---- 4. invariance and containment ------------------------------------------------------------------------------------------------
def slab_requests(m):
    return [(0, m), (1, m - 1), (15, 3), (16, 16), (17, m - 17), (0, 1), (m - 1, 1), (5, 0), (m, 0)]


@pytest.mark.parametrize("k,m,n", ((5, 37, 53), (40, 130, 257), (5, 17, 65)))
def test_rows_do_not_depend_on_the_request_or_the_panels(hip, k, m, n, monkeypatch):
    W, H = case(k, m, n)
    nb = (n + 7) // 8
    with context(hip, W, H) as ctx:
        whole = {"threshold": ctx.theta_bits(threshold=0.5).bits.copy(), "seed": ctx.theta_bits(seed=11).bits.copy()}
        assert whole["threshold"].any() and whole["seed"].any()
        for panel in (None, "1", "7", "16", "48"):
            if panel is not None:
                monkeypatch.setenv("NBMF_PREDICT_PANEL_ROWS", panel)
            for mode, arg in (("threshold", 0.5), ("seed", 11)):
                for row0, nrows in slab_requests(m):
                    if nrows < 0 or row0 + nrows > m:
                        continue
                    got = ctx.theta_bits(row0, nrows, **{mode: arg})
                    assert got.shape == (nrows, n)
                    assert np.array_equal(got.bits, whole[mode][row0:row0 + nrows]), (panel, mode, row0, nrows)
        # out as a column slice of a wider array: exactly ceil(n / 8) bytes of each requested row change
        for mode, arg in (("threshold", 0.5), ("seed", 11)):
            for row0, nrows in ((0, m), (16, min(17, m - 16)), (3, 0)):
                buf = np.full((m + 2, nb + 5), SENTINEL, dtype=np.uint8)
                out = buf[1:1 + nrows, 2:2 + nb]
                got = ctx.theta_bits(row0, nrows, out=out, **{mode: arg})
                assert np.array_equal(out, whole[mode][row0:row0 + nrows])
                assert np.array_equal(got.bits, out) and (nrows == 0 or np.shares_memory(got.bits, buf))
                buf[1:1 + nrows, 2:2 + nb] = SENTINEL
                assert np.all(buf == SENTINEL), "something outside the request was written"


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------------
def test_zero_one_and_nan_thetas(hip):
    k, m, n = 5, 37, 53
    comp = np.arange(m) % k
    W = np.zeros((k, m))
    W[comp, np.arange(m)] = 1.0                # one-hot columns: Theta[i] = H[comp[i]] exactly
    W[:, 6] = 0.0                              # row 6: Theta = 0
    H = np.random.default_rng(5).uniform(0.1, 0.9, (k, n))
    H[1] = 1.0                                 # rows with comp == 1: Theta = 1
    H[2] = 1.5                                 # rows with comp == 2: Theta = 1 after the clip, 1.5 without it
    ones_rows, over_rows = np.flatnonzero((comp == 1) & (np.arange(m) != 6)), np.flatnonzero((comp == 2) & (np.arange(m) != 6))
    full = packed(np.ones((1, n), dtype=bool))[0]          # (pad bits zero)
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        assert not theta[6].any() and np.all(theta[ones_rows] == 1.0) and np.all(theta[over_rows] == 1.0)
        for s in SEEDS + (7,):
            got = ctx.theta_bits(seed=s)
            assert not got.bits[6].any(), "theta = 0 drew a one"
            assert np.all(got.bits[ones_rows] == full) and np.all(got.bits[over_rows] == full), "theta = 1 missed a one"
            assert np.array_equal(got.toarray(), hip.hash_uniform(m, n, s) < theta)
        # without the clip the threshold sees 1.5, as the byte path does
        raw = ctx.predict_rows(clip_theta=False)
        assert np.all(raw[over_rows] == 1.5)
        for t in (1.0, 1.25, 1.5):
            want = ctx.predict_rows(clip_theta=False, threshold=t)
            assert np.array_equal(ctx.theta_bits(threshold=t, clip_theta=False).bits, packed(want))
            assert np.array_equal(want, raw > t)
        assert not ctx.theta_bits(threshold=1.0).bits.any()                 # clipped: nothing is above 1
        assert np.all(ctx.theta_bits(threshold=1.0, clip_theta=False).bits[over_rows] == full)
        assert np.array_equal(ctx.theta_bits(seed=3, clip_theta=False).toarray(), hip.hash_uniform(m, n, 3) < raw)
    Hn = H.copy()
    Hn[3, 10] = np.nan                          # column 10 of every row that has a weight on component 3 ... and 0 * NaN = NaN
    with context(hip, W, Hn) as ctx:
        theta = ctx.predict_rows()
        nan = np.isnan(theta)
        assert nan[:, 10].any() and not np.delete(nan, 10, axis=1).any()
        for kw in ({"threshold": -1.0}, {"threshold": 0.5}, {"seed": 0}, {"seed": 2 ** 64 - 1}):
            got = ctx.theta_bits(**kw).toarray()
            assert not got[nan].any(), f"{kw}: a NaN theta decided 1"
            with np.errstate(invalid="ignore"):
                want = theta > kw["threshold"] if "threshold" in kw else hip.hash_uniform(m, n, kw["seed"]) < theta
            assert np.array_equal(got, want)
        assert np.array_equal(ctx.theta_bits(threshold=-1.0).toarray(), ~nan)


# ---- 6. errors through the C ABI ----------------------------------------------------------------------------------------------------
@pytest.fixture()
def abi(hip):
    """(lib, ctx, out, good): a context with case 5's factors, a sentinel-filled 37 x 9 output, and the threshold-0.5 bytes;
    after the test the context must still give those bytes."""
    W, H = case(5)
    out = np.full((37, 9), SENTINEL, dtype=np.uint8)
    with context(hip, W, H) as ctx:
        good = ctx.theta_bits(threshold=0.5).bits.copy()
        yield hip.load(), ctx, out, good
        assert np.array_equal(ctx.theta_bits(threshold=0.5).bits, good), "the context is not usable after the error"


def test_ldout_too_small(hip, abi):
    lib, ctx, out, good = abi
    assert lib.nbmf_theta_bits(ctx._h, 0, 37, 1, hip.BITS_THRESHOLD, 0.5, 0, ptr(out), 6) == hip.NBMF_ERR_ARG
    assert b"ceil(n / 8)" in lib.nbmf_last_error() and np.all(out == SENTINEL)
    assert lib.nbmf_theta_bits(ctx._h, 0, 37, 1, hip.BITS_THRESHOLD, 0.5, 0, ptr(out), 9) == hip.NBMF_OK
    assert np.array_equal(out[:, :7], good) and np.all(out[:, 7:] == SENTINEL)


def test_unknown_mode(hip, abi):
    lib, ctx, out, good = abi
    for mode in (2, -1):
        assert lib.nbmf_theta_bits(ctx._h, 0, 37, 1, mode, 0.5, 0, ptr(out), 9) == hip.NBMF_ERR_ARG
        assert b"mode" in lib.nbmf_last_error() and np.all(out == SENTINEL)


def test_nan_threshold(hip, abi):
    lib, ctx, out, good = abi
    assert lib.nbmf_theta_bits(ctx._h, 0, 37, 1, hip.BITS_THRESHOLD, float("nan"), 0, ptr(out), 9) == hip.NBMF_ERR_ARG
    assert b"NaN" in lib.nbmf_last_error() and np.all(out == SENTINEL)
    with pytest.raises(ValueError, match="NaN"):
        ctx.theta_bits(threshold=float("nan"))
    # the threshold is not looked at in sample mode
    assert lib.nbmf_theta_bits(ctx._h, 0, 37, 1, hip.BITS_SAMPLE, float("nan"), 4, ptr(out), 9) == hip.NBMF_OK
    assert np.array_equal(out[:, :7], ctx.theta_bits(seed=4).bits)


def test_rows_and_null_output(hip, abi):
    lib, ctx, out, good = abi
    for row0, nrows in ((-1, 2), (37, 1), (36, 2), (0, -1), (38, 0)):
        assert lib.nbmf_theta_bits(ctx._h, row0, nrows, 1, hip.BITS_THRESHOLD, 0.5, 0, ptr(out), 9) == hip.NBMF_ERR_ARG
    assert lib.nbmf_theta_bits(ctx._h, 0, 37, 1, hip.BITS_THRESHOLD, 0.5, 0, None, 9) == hip.NBMF_ERR_ARG
    assert lib.nbmf_theta_bits(ctx._h, 5, 0, 1, hip.BITS_THRESHOLD, 0.5, 0, None, 9) == hip.NBMF_OK      # no rows: nothing touched
    assert np.all(out == SENTINEL)


def test_binding_wants_exactly_one_of_threshold_and_seed(hip, abi):
    lib, ctx, out, good = abi
    calls = (lambda: ctx.theta_bits(), lambda: ctx.theta_bits(threshold=0.5, seed=1), lambda: ctx.theta_bits(seed=-1),
             lambda: ctx.theta_bits(seed=2 ** 64), lambda: ctx.theta_bits(seed=True), lambda: ctx.theta_bits(seed=1.0),
             lambda: ctx.theta_bits(threshold=0.5, out=np.zeros((37, 6), dtype=np.uint8)),
             lambda: ctx.theta_bits(threshold=0.5, out=np.zeros((37, 7), dtype=np.int8)),
             lambda: ctx.theta_bits(threshold=0.5, out=np.zeros((37, 14), dtype=np.uint8)[:, ::2]),
             lambda: ctx.theta_bits(threshold=0.5, out=[[0] * 7] * 37), lambda: ctx.theta_bits(30, 8, threshold=0.5))
    for call in calls:
        with pytest.raises(ValueError):
            call()


def test_no_factors(hip):
    lib = hip.load()
    out = np.full((37, 7), SENTINEL, dtype=np.uint8)
    W, H = case(5)
    with hip.Context(37, 53, 5) as ctx:
        assert lib.nbmf_theta_bits(ctx._h, 0, 37, 1, hip.BITS_SAMPLE, 0.0, 1, ptr(out), 7) == hip.NBMF_ERR_STATE
        assert b"no factors" in lib.nbmf_last_error() and np.all(out == SENTINEL)
        with pytest.raises(hip.NBMFHipError, match="no factors"):
            ctx.theta_bits(seed=1)
        ctx.set_factors(W, H)
        assert np.array_equal(ctx.theta_bits(seed=1).toarray(), hip.hash_uniform(37, 53, 1) < ctx.predict_rows())


def test_sharded_context(hip):
    lib = hip.load()
    out = np.full((37, 7), SENTINEL, dtype=np.uint8)
    W, H = case(5)
    X = (np.random.default_rng(2).random((37, 53)) < 0.3).astype(np.float64)
    with hip.Context(37, 53, 5) as ctx:
        ctx.set_hyper(1.2, 1.2)
        ctx.upload(X)
        ctx.set_factors(W, H)
        ctx.comm_init_host(lambda arr: None, 1, 0)
        assert lib.nbmf_theta_bits(ctx._h, 0, 37, 1, hip.BITS_THRESHOLD, 0.5, 0, ptr(out), 7) == hip.NBMF_ERR_STATE
        assert b"unsharded" in lib.nbmf_last_error() and np.all(out == SENTINEL)
        ctx.comm_detach()
        assert np.array_equal(ctx.theta_bits(threshold=0.5).bits, packed(ctx.predict_rows(threshold=0.5)))


# ---- 7. the estimator ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orientation", ["beta-dir", "dir-beta"])
def test_estimator_predict_packed_and_sample(hip, orientation):
    from nbmf_mm_amd import NBMF, PackedBits
    g = np.random.default_rng(11)
    X = (g.random((60, 80)) < 0.3).astype(np.float64)
    model = NBMF(4, random_state=0, max_iter=30, tol=0, orientation=orientation).fit(X)
    theta = model.predict_proba()

    for t in (0.5, 0.3):
        bits = model.predict(threshold=t, packed=True)
        assert isinstance(bits, PackedBits) and bits.shape == (60, 80)
        assert np.array_equal(bits.toarray(), model.predict(threshold=t))
    assert 0.1 < model.predict(threshold=0.3, packed=True).toarray().mean() < 0.9

    want = hip.hash_uniform(60, 80, 3) < theta
    drawn = model.sample(random_state=3)
    assert drawn.dtype == np.bool_ and drawn.shape == (60, 80)
    assert np.array_equal(drawn, want)
    as_bits = model.sample(random_state=3, packed=True)
    assert isinstance(as_bits, PackedBits) and np.array_equal(as_bits.toarray(), want)
    assert not np.array_equal(model.sample(random_state=4), want)
    assert model.sample().shape == (60, 80)                                  # a seed from the global RNG

    Wnew = model.transform(X[:7])
    assert np.array_equal(model.sample(W=Wnew, random_state=3), hip.hash_uniform(7, 80, 3) < model.predict_proba(W=Wnew))
    assert np.array_equal(model.predict(W=Wnew, packed=True).toarray(), model.predict(W=Wnew))

    # the parametric bootstrap: a fit of the bits is the fit of the matrix they hold
    rep = model.sample(random_state=0, packed=True)
    a = NBMF(n_components=3, max_iter=5, random_state=0, orientation=orientation).fit(rep)
    b = NBMF(n_components=3, max_iter=5, random_state=0, orientation=orientation).fit(rep.toarray())
    assert len(a.loss_curve_) > 0 and np.array_equal(np.asarray(a.loss_curve_), np.asarray(b.loss_curve_))
