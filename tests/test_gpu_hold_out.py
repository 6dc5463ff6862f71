"""The held-out split drawn on the device: nbmf_hold_out, nbmf_hold_out_undo, nbmf_get_eval_pairs (Context.hold_out,
hold_out_undo, eval_pairs), NBMF.fit(holdout=...) and experiments.cross_validate.

REFERENCE.  ``_hip.holdout_reference`` (NumPy; tests/test_hold_out_cpu.py checks it on its own) says which entries are held
out; the HOST ROUTE it replaces -- a second context uploaded with ``mask & ~held`` and given the pairs ``np.nonzero`` finds
through ``set_eval`` -- says what every later call must compute.  The feature moves entries and adds no arithmetic: every
comparison here is exact, in integers or bit for bit.

SHAPES.  37 x 83 (ragged in both dimensions, several 16-blocks, rows longer than one wave) with K = 5, 64 and 130; 16 x 16;
1 x 1; 64 x 128 (a multiple of the tile in both dimensions); 100 x 500 with K = 6 and 512 x 512 with K = 64 for the fits.  Every
case takes milliseconds."""
import numpy as np
import pytest

from conftest import config1_X, config1_mask, midsize_XM
from test_hold_out_cpu import narrow_interval_37x83

pytestmark = pytest.mark.gpu

MAX_SEED = 2 ** 64 - 1


@pytest.fixture(scope="module")
def hip():
    from nbmf_mm_amd import _hip
    assert _hip.device_count() >= 1, "no MI355X visible: the GPU tests must run on the GPU box"
    return _hip


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def data(shape, density=0.3, observed=0.8, seed=0):
    """The user's binary matrix (float64) and its observed pattern (bool)."""
    g = np.random.default_rng([seed, *shape])
    return (g.random(shape) < density).astype(np.float64), g.random(shape) < observed


def init(m, n, k, seed=12345):
    from nbmf_mm_amd.experiments import _init
    return _init(m, n, k, seed)


def internal(a, transposed):
    return np.ascontiguousarray(a.T) if transposed else a


def host_pairs(X, held, transposed):
    """What eval_pairs of the host route gives: the held-out entries in row-major order of the internal layout, and X there."""
    r, c = np.nonzero(internal(held, transposed))
    return r.astype(np.int64), c.astype(np.int64), internal(X, transposed)[r, c].astype(np.uint8)


def assert_list(hip, ctx, X, M, transposed, seed, lo, hi):
    """hold_out on ``ctx`` (which holds X under M) against the reference; leaves the hold-out in place.  Returns the count."""
    held = hip.holdout_reference(X.shape, seed, lo, hi, mask=M)
    r, c, x = host_pairs(X, held, transposed)
    before = ctx.n_obs()
    count = ctx.hold_out(seed, lo, hi, transposed=transposed)
    rows, cols, truth = ctx.eval_pairs()
    assert count == r.size == rows.size
    assert rows.dtype == cols.dtype == np.int64 and truth.dtype == np.uint8
    assert np.array_equal(rows, r) and np.array_equal(cols, c) and np.array_equal(truth, x)
    assert ctx.n_obs() == before - count
    return count


def run_all(ctx, W0, H0, iters=12, tol=0.0):
    ctx.set_factors(W0, H0)
    losses, n_iter = ctx.run(iters, tol)
    return (losses, n_iter) + ctx.get_factors()


def assert_same_run(a, b):
    assert a[1] == b[1] and same_bits(a[0], b[0]) and same_bits(a[2], b[2]) and same_bits(a[3], b[3])


def assert_same_eval(ctx_a, ctx_b):
    ca, cb = ctx_a.eval_curve(), ctx_b.eval_curve()
    assert np.array_equal(ca[0], cb[0]) and same_bits(ca[1], cb[1]) and ca[2:] == cb[2:]
    for fa, fb in zip(ctx_a.best_factors(), ctx_b.best_factors()):
        assert same_bits(fa, fb)


INTERVALS = [(0.0, 0.25), (0.4, 0.6)]


# ---- 1. the list ---------------------------------------------------------------------------------------------------------
def upload_as(hip, ctx, path, X, M, transposed):
    """Put X (observed under M, or everywhere with M None) on ``ctx`` by the named ingest path."""
    import scipy.sparse as sp
    from nbmf_mm_amd import PackedBits
    from nbmf_mm_amd._solver import upload_any
    if path == "float64":
        assert ctx.upload(X, mask=None if M is None else M.astype(np.float64), transposed=transposed)
    elif path == "uint8":
        assert ctx.upload(X.astype(np.uint8), mask=M, transposed=transposed)
    elif path == "packed":
        assert ctx.upload(PackedBits.from_dense(X != 0), mask=None if M is None else PackedBits.from_dense(M), transposed=transposed)
    elif path == "csr":
        assert upload_any(ctx, sp.csr_matrix(X), None if M is None else sp.csr_matrix(M.astype(np.float64)), transposed=transposed)
    else:
        raise AssertionError(path)


@pytest.mark.parametrize("masked", [False, True], ids=["no-mask", "mask"])
@pytest.mark.parametrize("transposed", [False, True], ids=["beta-dir", "dir-beta"])
@pytest.mark.parametrize("path", ["float64", "uint8", "packed", "csr"])
def test_list_on_every_ingest_path(hip, path, transposed, masked):
    X, M = data((37, 83))
    M = M if masked else None
    m, n = (83, 37) if transposed else (37, 83)
    with hip.Context(m, n, 5) as ctx:
        upload_as(hip, ctx, path, X, M, transposed)
        n_obs = ctx.n_obs()
        for seed in (0, MAX_SEED):
            for lo, hi in INTERVALS:
                count = assert_list(hip, ctx, X, M, transposed, seed, lo, hi)
                assert 0 < count < n_obs
                ctx.hold_out_undo()
                assert ctx.n_obs() == n_obs and ctx.eval_pairs()[0].size == 0


@pytest.mark.parametrize("transposed", [False, True], ids=["beta-dir", "dir-beta"])
def test_list_on_generated_data(hip, transposed):
    m, n = 37, 83
    Y, obs = hip.synthetic_reference(m, n, 9, density=0.3, observed=0.8)      # the internal matrix
    X, M = (Y.T, obs.T) if transposed else (Y, obs)                           # the user's, whose counters the rule uses
    with hip.Context(m, n, 5) as ctx:
        ctx.generate(9, density=0.3, observed=0.8)
        assert ctx.n_obs() == obs.sum()
        for seed in (0, MAX_SEED):
            for lo, hi in INTERVALS:
                assert_list(hip, ctx, X, M, transposed, seed, lo, hi)
                ctx.hold_out_undo()


@pytest.mark.parametrize("shape", [(16, 16), (64, 128), (37, 83), (3, 1100)])
def test_list_shapes_and_special_intervals(hip, shape):
    X, M = data(shape, observed=0.6)
    for transposed in (False, True):
        m, n = shape[::-1] if transposed else shape
        with hip.Context(m, n, 5) as ctx:
            ctx.upload(X.astype(np.uint8), mask=M, transposed=transposed)
            for lo, hi in INTERVALS + [(0.0, 1.0 / 3), (0.75, 1.0)]:
                assert_list(hip, ctx, X, M, transposed, 7, lo, hi)
                ctx.hold_out_undo()


def test_rows_that_hold_out_nothing_and_rows_held_out_whole(hip):
    shape = (37, 83)
    seed, lo, hi = narrow_interval_37x83()
    X, _ = data(shape)
    for transposed in (False, True):
        m, n = shape[::-1] if transposed else shape
        with hip.Context(m, n, 5) as ctx:
            # so narrow that several rows hold out nothing
            ctx.upload(X, transposed=transposed)
            count = assert_list(hip, ctx, X, None, transposed, seed, lo, hi)
            rows = ctx.eval_pairs()[0]
            assert count >= 1 and np.setdiff1d(np.arange(m), rows).size >= 3
            ctx.hold_out_undo()
            # a sparse mask and a wide interval: whole rows of the internal matrix lose every observed entry
            M = np.random.default_rng(3).random(shape) < 0.04
            held = internal(hip.holdout_reference(shape, 1, 0.0, 0.7, mask=M), transposed)
            Mi = internal(M, transposed)
            assert np.count_nonzero((Mi.sum(axis=1) > 0) & ((Mi & ~held).sum(axis=1) == 0)) >= 3
            ctx.upload(X, mask=M, transposed=transposed)
            assert_list(hip, ctx, X, M, transposed, 1, 0.0, 0.7)
            ctx.hold_out_undo()
            assert ctx.n_obs() == M.sum()


# ---- 2. the images: everything behind the hold-out is the host route's, bit for bit ---------------------------------------
def assert_images(hip, X, M, k, transposed, seed, lo, hi, every=5, patience=0, iters=12):
    m, n = X.shape[::-1] if transposed else X.shape
    W0, H0 = init(m, n, k)
    held = hip.holdout_reference(X.shape, seed, lo, hi, mask=M)
    with hip.Context(m, n, k) as dev, hip.Context(m, n, k) as host:
        dev.upload(X, mask=M, transposed=transposed)
        count = dev.hold_out(seed, lo, hi, transposed=transposed, every=every, patience=patience)
        host.upload(X, mask=~held if M is None else M & ~held, transposed=transposed)
        host.set_eval(*host_pairs(X, held, transposed), every=every, patience=patience)
        assert count == held.sum() and dev.n_obs() == host.n_obs()
        assert_same_run(run_all(dev, W0, H0, iters), run_all(host, W0, H0, iters))
        assert_same_eval(dev, host)
        assert same_bits(dev.eval_loglik(), host.eval_loglik())
        assert same_bits(dev.loss(), host.loss()) and same_bits(dev.loglik_strict(), host.loglik_strict())


@pytest.mark.parametrize("masked", [False, True], ids=["no-mask", "mask"])
@pytest.mark.parametrize("k", [5, 64, 130])
def test_images_match_the_host_route(hip, k, masked):
    X, M = data((37, 83))
    for transposed in (False, True):
        assert_images(hip, X, M if masked else None, k, transposed, 11, 0.0, 0.25)
    assert_images(hip, X, M if masked else None, k, False, MAX_SEED, 0.4, 0.6, every=3, patience=2)


def test_images_match_the_host_route_at_the_fit_shapes(hip):
    assert_images(hip, config1_X(), config1_mask(), 6, False, 5, 0.0, 0.2, every=5, patience=0, iters=20)
    assert_images(hip, config1_X(), None, 6, True, 5, 0.4, 0.6, every=5, patience=0, iters=20)
    X, M = midsize_XM()
    assert_images(hip, X, M != 0, 64, False, 5, 0.0, 0.1, every=5, patience=0, iters=10)


# ---- 3. the undo -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["no-mask", "mask"])
@pytest.mark.parametrize("k", [5, 64])
def test_undo_gives_the_uploaded_context_back(hip, k, masked):
    X, M = data((37, 83))
    M = M if masked else None
    m, n = X.shape
    W0, H0 = init(m, n, k)
    with hip.Context(m, n, k) as ctx, hip.Context(m, n, k) as fresh:
        fresh.upload(X, mask=M)
        full = hip.variant_stats()[0]
        want = run_all(fresh, W0, H0)
        fresh_full = hip.variant_stats()[0] - full
        ctx.upload(X, mask=M)
        n_obs = ctx.n_obs()
        ctx.hold_out(3, 0.0, 0.25)
        full = hip.variant_stats()[0]
        run_all(ctx, W0, H0)
        assert hip.variant_stats()[0] == full                   # something is unobserved: never the two-state W sweep
        ctx.hold_out_undo()
        assert ctx.n_obs() == n_obs
        full = hip.variant_stats()[0]
        assert_same_run(run_all(ctx, W0, H0), want)
        undone_full = hip.variant_stats()[0] - full
        assert undone_full == fresh_full
        if k == 64 and not masked:    # K = 64 runs on the launches; 83 % 16 != 0: the pad marks of image B are back
            assert undone_full > 0
        assert same_bits(ctx.loss(), fresh.loss()) and same_bits(ctx.loglik_strict(), fresh.loglik_strict())


def test_five_folds_in_sequence_are_five_fresh_contexts(hip):
    X, M = data((37, 83))
    m, n, k = 37, 83, 5
    W0, H0 = init(m, n, k)

    def fold(ctx, f):
        count = ctx.hold_out(2, f / 5, (f + 1) / 5, every=4)
        out = run_all(ctx, W0, H0)
        return count, out, ctx.eval_curve(), ctx.best_factors(), ctx.eval_pairs()

    with hip.Context(m, n, k) as ctx:
        ctx.upload(X, mask=M)
        counts = []
        for f in range(5):
            got = fold(ctx, f)
            ctx.hold_out_undo()
            with hip.Context(m, n, k) as fresh:
                fresh.upload(X, mask=M)
                want = fold(fresh, f)
            assert got[0] == want[0]
            assert_same_run(got[1], want[1])
            assert np.array_equal(got[2][0], want[2][0]) and same_bits(got[2][1], want[2][1]) and got[2][2:] == want[2][2:]
            assert all(same_bits(a, b) for a, b in zip(got[3], want[3]))
            assert all(np.array_equal(a, b) for a, b in zip(got[4], want[4]))
            counts.append(got[0])
        assert sum(counts) == M.sum() == ctx.n_obs()


# ---- 4. state rules ----------------------------------------------------------------------------------------------------------
def test_empty_splits_change_nothing(hip):
    X, M = data((16, 16))
    m, n, k = 16, 16, 5
    W0, H0 = init(m, n, k)
    nothing = (0.5, 0.5 + 2.0 ** -40)
    assert not hip.holdout_reference((m, n), 0, *nothing, mask=M).any()
    rows, cols = np.array([3, 0, 15]), np.array([1, 15, 0])
    x = X[rows, cols].astype(np.uint8)
    with hip.Context(m, n, k) as ctx, hip.Context(m, n, k) as twin:
        for c in (ctx, twin):
            c.upload(X, mask=M)
            c.set_eval(rows, cols, x, every=3, patience=0)
        with pytest.raises(ValueError, match="holds out no entry"):
            ctx.hold_out(0, *nothing)
        with pytest.raises(ValueError, match="leaves no observed entry"):
            ctx.hold_out(0, 0.0, 1.0)
        for bad in ((0.5, 0.5), (0.6, 0.4), (-0.1, 0.5), (0.0, 1.5), (float("nan"), 0.5)):
            with pytest.raises(ValueError, match="interval"):
                ctx.hold_out(0, *bad)
        with pytest.raises(ValueError, match="every"):
            ctx.hold_out(0, 0.0, 0.5, every=0)
        with pytest.raises(ValueError, match="patience"):
            ctx.hold_out(0, 0.0, 0.5, patience=-1)
        assert ctx.n_obs() == M.sum()
        got = ctx.eval_pairs()
        assert np.array_equal(got[0], rows) and np.array_equal(got[1], cols) and np.array_equal(got[2], x)
        assert_same_run(run_all(ctx, W0, H0), run_all(twin, W0, H0))
        assert_same_eval(ctx, twin)
        ctx.set_eval(rows[:0], cols[:0], x[:0])                 # a plain eval set can still be dropped
    with hip.Context(1, 1, 1) as ctx:
        ctx.upload(np.ones((1, 1)))
        with pytest.raises(ValueError, match="leaves no observed entry"):
            ctx.hold_out(0, 0.0, 1.0)
        assert ctx.n_obs() == 1 and ctx.eval_pairs()[0].size == 0


def test_state_rules(hip):
    X, M = data((37, 83))
    m, n, k = 37, 83, 5
    W0, H0 = init(m, n, k)
    with hip.Context(m, n, k) as ctx:
        with pytest.raises(hip.NBMFHipError, match="hold-out needs binary data with a binary or no mask"):
            ctx.hold_out(0, 0.0, 0.5)                           # nothing uploaded
        with pytest.raises(hip.NBMFHipError, match="no hold-out in place"):
            ctx.hold_out_undo()
        ctx.upload(X, mask=M)
        with pytest.raises(hip.NBMFHipError, match="no hold-out in place"):
            ctx.hold_out_undo()
        count = ctx.hold_out(0, 0.0, 0.5)                       # needs no factors
        with pytest.raises(hip.NBMFHipError, match="undo it first"):
            ctx.hold_out(1, 0.5, 1.0)
        pairs = ctx.eval_pairs()
        for cnt in (3, 0):
            with pytest.raises(hip.NBMFHipError, match="nbmf_hold_out_undo first"):
                ctx.set_eval(pairs[0][:cnt], pairs[1][:cnt], pairs[2][:cnt])
        assert ctx.eval_pairs()[0].size == count
        with pytest.raises(hip.NBMFHipError, match="eval set"):
            ctx.run_batch([1.2], [1.2], W0, H0, 5, 0.0)
        # a new upload forgets the hold-out; the list stays as a plain eval set
        ctx.upload(X, mask=M)
        assert ctx.n_obs() == M.sum() and ctx.eval_pairs()[0].size == count
        with pytest.raises(hip.NBMFHipError, match="no hold-out in place"):
            ctx.hold_out_undo()
        ctx.set_eval(pairs[0][:0], pairs[1][:0], pairs[2][:0])
        assert ctx.eval_pairs()[0].size == 0
        # a communicator and a hold-out do not go together
        ctx.comm_init_host(lambda arr: None, 1, 0, 0)
        with pytest.raises(hip.NBMFHipError, match="unsharded"):
            ctx.hold_out(0, 0.0, 0.5)
        ctx.comm_detach()
        # the real-valued storage paths
        ctx.set_storage("f64")
        ctx.upload(X, mask=M)
        with pytest.raises(hip.NBMFHipError, match="hold-out needs binary data with a binary or no mask"):
            ctx.hold_out(0, 0.0, 0.5)
        ctx.set_storage("auto")
        ctx.upload(X, mask=np.where(M, 0.5, 0.0))
        with pytest.raises(hip.NBMFHipError, match="hold-out needs binary data with a binary or no mask"):
            ctx.hold_out(0, 0.0, 0.5)
        ctx.upload(X, mask=M)
        assert ctx.hold_out(0, 0.0, 0.5) == count


# ---- 5. the estimator ----------------------------------------------------------------------------------------------------------
FIT_ATTRS = ("W_", "components_", "loss_curve_", "eval_loglik_", "eval_perplexity_")


def assert_same_fit(a, b):
    for name in FIT_ATTRS:
        assert same_bits(getattr(a, name), getattr(b, name)), name
    assert a.n_iter_ == b.n_iter_ and a.best_iter_ == b.best_iter_ and a.stopped_early_ == b.stopped_early_
    assert np.array_equal(a.eval_iters_, b.eval_iters_) and a.loss_ == b.loss_


@pytest.mark.parametrize("patience", [0, 3])
@pytest.mark.parametrize("orientation", ["beta-dir", "dir-beta"])
def test_fit_with_holdout_is_fit_with_the_host_masks(hip, orientation, patience):
    from nbmf_mm_amd import NBMF, PackedBits, holdout_mask
    X, M = config1_X(), config1_mask()
    make = lambda: NBMF(n_components=6, max_iter=60, tol=1e-7, random_state=7, orientation=orientation)   # noqa: E731
    for h, s in ((0.2, 3), ((0.4, 0.6), MAX_SEED)):
        held = holdout_mask(X.shape, s, h, mask=M)
        want = make().fit(X, mask=M & ~held, eval_mask=held, eval_every=5, patience=patience)
        got = make().fit(X, mask=M, holdout=h, holdout_seed=s, eval_every=5, patience=patience)
        assert_same_fit(got, want)
        assert got.holdout_seed_ == s and got.holdout_count_ == held.sum()
        assert got.holdout_interval_ == hip.holdout_interval(h)
        assert not hasattr(want, "holdout_seed_")
    packed = make().fit(PackedBits.from_dense(X != 0), mask=M, holdout=(0.4, 0.6), holdout_seed=MAX_SEED, eval_every=5,
                        patience=patience)
    assert_same_fit(packed, got)
    # no mask: the pool is everything
    held = holdout_mask(X.shape, 3, 0.2)
    assert_same_fit(make().fit(X, holdout=0.2, holdout_seed=3, eval_every=5, patience=patience),
                    make().fit(X, mask=~held, eval_mask=held, eval_every=5, patience=patience))


def test_fit_seed_default_restarts_and_attributes(hip):
    from nbmf_mm_amd import NBMF
    X, M = config1_X(), config1_mask()
    make = lambda **kw: NBMF(n_components=6, max_iter=30, tol=1e-7, random_state=7, **kw)   # noqa: E731
    a = make().fit(X, mask=M, holdout=0.2, eval_every=5)
    b = make().fit(X, mask=M, holdout=0.2, holdout_seed=7, eval_every=5)
    assert a.holdout_seed_ == b.holdout_seed_ == 7
    assert_same_fit(a, b)
    # restarts: one after the other on the same split; the kept one is a single fit with its seed and that split
    r = make(n_init=2).fit(X, mask=M, holdout=0.2, eval_every=5)
    assert r.holdout_seed_ == 7
    singles = [NBMF(n_components=6, max_iter=30, tol=1e-7, random_state=7 + i).fit(X, mask=M, holdout=0.2, holdout_seed=7, eval_every=5)
               for i in range(2)]
    assert_same_fit(r, min(singles, key=lambda s: s.loss_))
    # without a random_state the seed is drawn, and reported
    c = NBMF(n_components=6, max_iter=10).fit(X, holdout=0.2)
    assert 0 <= c.holdout_seed_ < 2 ** 64 and c.holdout_interval_ == (0.0, 0.2)
    # gone after a later plain fit
    a.fit(X, mask=M)
    for name in ("holdout_seed_", "holdout_interval_", "holdout_count_", "eval_iters_", "best_iter_"):
        assert not hasattr(a, name)
    # data the library does not hold as byte codes: its own words, as a ValueError
    with pytest.raises(ValueError, match="hold-out needs binary data with a binary or no mask"):
        make().fit(np.random.default_rng(0).random((20, 30)), holdout=0.2)
    with pytest.raises(ValueError, match="leaves no observed entry"):
        make().fit(X, holdout=(0.0, 1.0))


# ---- 6. cross-validation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orientation", ["beta-dir", "dir-beta"])
def test_cross_validate(hip, orientation):
    from nbmf_mm_amd import NBMF
    from nbmf_mm_amd.experiments import cross_validate
    X, M = config1_X(), config1_mask()
    kw = dict(alpha=1.1, beta=1.3, max_iter=40, tol=1e-7, eval_every=5, patience=2)
    folds = cross_validate(X, 6, n_folds=3, mask=M, seed=4, random_state=12345, orientation=orientation, **kw)
    assert [r["fold"] for r in folds] == [0, 1, 2]
    assert sum(r["count"] for r in folds) == M.sum()
    for f, row in enumerate(folds):
        # (the module's init rule IS the solver's draw under random_state: the same start)
        one = NBMF(n_components=6, alpha=1.1, beta=1.3, max_iter=40, tol=1e-7, random_state=12345, orientation=orientation).fit(
            X, mask=M, holdout=(f / 3, (f + 1) / 3), holdout_seed=4, eval_every=5, patience=2)
        assert row["count"] == one.holdout_count_ and row["n_iter"] == one.n_iter_ and row["loss"] == one.loss_
        assert np.array_equal(row["eval_iters"], one.eval_iters_) and same_bits(row["eval_loglik"], one.eval_loglik_)
        assert row["perplexity"] == one.eval_perplexity_[-1]
        assert row["best_iter"] == one.best_iter_ and row["stopped_early"] == one.stopped_early_
        assert row["best_perplexity"] == one.eval_perplexity_[list(one.eval_iters_).index(one.best_iter_)]
    # no mask, PackedBits data: the same folds as the dense matrix
    from nbmf_mm_amd import PackedBits
    a = cross_validate(X, 6, n_folds=2, seed=4, max_iter=10, orientation=orientation)
    b = cross_validate(PackedBits.from_dense(X != 0), 6, n_folds=2, seed=4, max_iter=10, orientation=orientation)
    assert sum(r["count"] for r in a) == X.size
    assert all(ra["count"] == rb["count"] and ra["loss"] == rb["loss"] and same_bits(ra["eval_loglik"], rb["eval_loglik"])
               for ra, rb in zip(a, b))
