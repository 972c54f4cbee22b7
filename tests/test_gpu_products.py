"""GPU: every instance of the dense and X^T Y products (csrc/rec_dense.hip, rec_dense_h2.hip) against plain float64, with the
instance asserted through mava_debug_rec_product_last_instance(); their column-block arguments (x_ld, ldw, y_ld, accumulate,
slab_stride) with NaN in everything a block must not use; launches whose blocks own 1, 2 and 5 tiles, or none; the gather's
wrap; and the refusals, which must launch nothing.  tests/product_instances.py holds the tables and the restated dispatch."""
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from tests import product_instances as P
from tests.conftest import assert_close
from tests.product_instances import Refusal, from_t32, to_t32

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = 12345.0


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@contextmanager
def _ctx(mode):
    from mava_amd._lib import Ctx

    cx = Ctx(mode)  # the arithmetic mode lives in a context handle
    try:
        yield cx.handle
    finally:
        cx.close()


def _inst():
    from mava_amd._lib import lib

    return lib().mava_debug_rec_product_last_instance()


def _last_error():
    from mava_amd._lib import lib

    return lib().mava_last_error().decode("utf-8", "replace")


def _p(t, offset_floats=0):
    return None if t is None else t.data_ptr() + 4 * offset_floats


def _dense(h, x, x_ld, w, ldw, b, g, y, y_ld, K, N, rows, relu, accumulate=0, gather=None):
    """One mava_rec_dense_f32 call; x, w, b, g, y are device addresses.  gather = (idx address, Rm, E, A, share): row-major x."""
    from mava_amd._lib import lib, stream_ptr

    rm, (idx, Rm, E, A, share) = (0, (None, 0, 0, 0, 1)) if gather is None else (1, gather)
    return lib().mava_rec_dense_f32(h, x, rm, idx, Rm, E, A, share, x_ld, int(accumulate), w, ldw, b, g, y, y_ld, K, N, rows, int(relu),
                                    stream_ptr())


def _xty(h, x, x_ld, y, y_ld, y_tail, y_split, y_tail_ld, K, N, rows, want_bias, scale, slab, n_slab, gather=None, slab_stride=None):
    from mava_amd._lib import lib, stream_ptr

    rm, (idx, Rm, E, A, share) = (0, (None, 0, 0, 0, 1)) if gather is None else (1, gather)
    return lib().mava_rec_xty_f32(h, x, rm, idx, Rm, E, A, share, x_ld, y, y_ld, y_tail, y_split, y_tail_ld, K, N, rows, int(want_bias),
                                  float(scale), slab.data_ptr(), slab.shape[1] if slab_stride is None else slab_stride, n_slab, stream_ptr())


def _ok(rc, what):
    from mava_amd._lib import check

    check(rc, what)
    torch.cuda.synchronize()


def _close(got, want, tol, name):
    got = np.asarray(got)
    assert np.isfinite(got).all(), f"{name}: {int((~np.isfinite(got)).sum())} elements not written or not finite"
    assert_close(got, want, tol, name)


SLACK = 384 * 32  # floats behind every output: a store past the last feature of the last tile lands here, and is seen


def _out(init, dev):
    """A device output buffer holding `init` (flat), followed by SLACK sentinel floats."""
    return torch.cat([_t(np.asarray(init, np.float32).reshape(-1), dev), torch.full((SLACK,), SENTINEL, device=dev)])


def _main(y):
    """The output proper, after checking that nothing was written behind it."""
    a = y.cpu().numpy()
    assert (a[-SLACK:] == SENTINEL).all(), "stores behind the end of the output"
    return a[:-SLACK]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


# ------------------------------------------------------------------------------------------ a. every instance once
@pytest.mark.parametrize("mode,c", P.dense_runs(), ids=lambda v: v if isinstance(v, str) else P.case_id(v))
def test_dense_instance_matches_float64(dev, mode, c):
    d = P.dense_data(c)
    K, N, rows = c.K, c.N, c.rows
    want_inst = P.predict_dense(mode, K, N, c.rowmajor, c.bias)
    assert not isinstance(want_inst, Refusal)
    w_d = _t(d["w"], dev)
    b_d = _t(d["b"], dev) if c.bias else None
    g_d = _t(to_t32(d["g"]), dev) if c.gate else None
    y = _out(np.full(rows * N, np.nan), dev)  # every element must be overwritten
    with _ctx(mode) as h:
        if c.rowmajor:
            src_d, idx_d = _t(d["src"], dev), _t(d["idx"], dev)
            rc = _dense(h, _p(src_d), K, _p(w_d), N, _p(b_d), _p(g_d), _p(y), 0, K, N, rows, c.relu,
                        gather=(_p(idx_d), d["Rm"], P.GATHER_E, P.GATHER_A, 1))
        else:
            x_d = _t(to_t32(d["x"]), dev)
            rc = _dense(h, _p(x_d), K, _p(w_d), N, _p(b_d), _p(g_d), _p(y), 0, K, N, rows, c.relu)
        _ok(rc, "dense")
    assert _inst() == want_inst, f"instance {_inst()} ran, the dispatch restatement says {want_inst}"
    _close(from_t32(_main(y), rows, N), d["want"], 1e-5, f"dense {mode} {c}")


@pytest.mark.parametrize("mode,c", P.xty_runs(), ids=lambda v: v if isinstance(v, str) else P.case_id(v))
def test_xty_instance_matches_float64(dev, mode, c):
    d = P.xty_data(c)
    K, N, rows = c.K, c.N, c.rows
    want_inst = P.predict_xty(mode, K, N, c.rowmajor, c.n_slab, rows // 32)
    assert not isinstance(want_inst, Refusal)
    used = K * N + (N if c.want_bias else 0)
    slab = torch.full((c.n_slab, used + 5), SENTINEL, device=dev)
    yv = d["y"]
    tail_d, split, tail_ld = None, 0, 0
    if c.y_split:  # the head matrix holds something else from y_split on
        head = yv.copy()
        head[:, c.y_split:] = NAN
        y_d = _t(to_t32(head), dev)
        tail_d, split, tail_ld = _t(to_t32(np.ascontiguousarray(yv[:, c.y_split:])), dev), c.y_split, N - c.y_split
    else:
        y_d = _t(to_t32(yv), dev)
    with _ctx(mode) as h:
        if c.rowmajor:
            src_d, idx_d = _t(d["src"], dev), _t(d["idx"], dev)
            rc = _xty(h, _p(src_d), K, _p(y_d), 0, _p(tail_d), split, tail_ld, K, N, rows, c.want_bias, c.scale, slab, c.n_slab,
                      gather=(_p(idx_d), d["Rm"], P.GATHER_E, P.GATHER_A, 1))
        else:
            x_d = _t(to_t32(d["x"]), dev)
            rc = _xty(h, _p(x_d), K, _p(y_d), 0, _p(tail_d), split, tail_ld, K, N, rows, c.want_bias, c.scale, slab, c.n_slab)
        _ok(rc, "xty")
    assert _inst() == want_inst, f"instance {_inst()} ran, the dispatch restatement says {want_inst}"
    s = slab.cpu().numpy()
    assert (s[:, used:] == SENTINEL).all(), "a slab row is written behind K N (+ N)"
    assert (s[:, :used] != SENTINEL).all(), "every block writes its whole slab row"
    tot = s[:, :used].astype(np.float64).sum(0)
    _close(tot[: K * N].reshape(K, N), d["dw"], 1e-5, f"xty dW {mode} {c}")
    if c.want_bias:
        _close(tot[K * N:], d["db"], 1e-5, f"xty db {mode} {c}")


# ------------------------------------------------------------------------------------------ b. column blocks
def _vec_poisoned(v, sl):
    out = np.full(v.shape, np.nan, np.float32)
    out[sl] = v[sl]
    return out


@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("blk", P.DENSE_BLOCKS, ids=P.case_id)
def test_dense_column_block_is_exact_and_stays_inside(dev, mode, blk):
    W = P.wide_data()
    rows, KX, NY = P.WIDE_ROWS, P.WIDE_K, P.WIDE_N
    k0, K, n0, N = blk.k0, blk.K, blk.n0, blk.N
    ks, ns = slice(k0, k0 + K), slice(n0, n0 + N)
    want_inst = P.predict_dense(mode, K, N, False, blk.bias)
    # NaN in everything the block must not use; without accumulate also in the y block, which is overwritten and not read
    y0 = W["y_old"].copy()
    if not blk.accumulate:
        y0[:, ns] = np.nan
    x_d = _t(to_t32(P.poisoned(W["x"], None, ks)), dev)
    w_d = _t(P.poisoned(W["w"], ks, ns), dev)
    b_d = _t(_vec_poisoned(W["b"], ns), dev) if blk.bias else None
    g_d = _t(to_t32(P.poisoned(W["g"], None, ns)), dev) if blk.gate else None
    y_d = _out(to_t32(y0), dev)
    # the same call on contiguous copies of the operands
    xc_d = _t(to_t32(np.ascontiguousarray(W["x"][:, ks])), dev)
    wc_d = _t(np.ascontiguousarray(W["w"][ks, ns]), dev)
    bc_d = _t(np.ascontiguousarray(W["b"][ns]), dev) if blk.bias else None
    gc_d = _t(to_t32(np.ascontiguousarray(W["g"][:, ns])), dev) if blk.gate else None
    yc_d = _out(to_t32(np.ascontiguousarray(y0[:, ns])), dev)
    with _ctx(mode) as h:
        _ok(_dense(h, _p(x_d, 32 * k0), KX, _p(w_d, k0 * NY + n0), NY, _p(b_d, n0), _p(g_d, 32 * n0), _p(y_d, 32 * n0), NY, K, N, rows,
                   blk.relu, blk.accumulate), "dense block")
        assert _inst() == want_inst
        _ok(_dense(h, _p(xc_d), K, _p(wc_d), N, _p(bc_d), _p(gc_d), _p(yc_d), N, K, N, rows, blk.relu, blk.accumulate), "dense contiguous")
        assert _inst() == want_inst, "the block and its contiguous copy run the same instance"
    got = from_t32(_main(y_d), rows, NY)
    want = P.dense_reference(W["x"][:, ks], W["w"][ks, ns], W["b"][ns] if blk.bias else None, blk.relu, W["g"][:, ns] if blk.gate else None,
                             W["y_old"][:, ns] if blk.accumulate else None)
    _close(got[:, ns], want, 1e-5, f"dense block {mode} {blk}")
    assert np.array_equal(_bits(got[:, ns]), _bits(from_t32(_main(yc_d), rows, N))), "block == contiguous call, bit for bit"
    outside = np.ones((rows, NY), bool)
    outside[:, ns] = False
    assert np.array_equal(_bits(got)[outside], _bits(y0)[outside]), "y outside the block is untouched"


@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("blk", P.XTY_BLOCKS, ids=P.case_id)
def test_xty_column_block_is_exact_and_stays_inside(dev, mode, blk):
    W = P.wide_data()
    rows, KX, NY = P.WIDE_ROWS, P.WIDE_K, P.WIDE_N
    k0, K, n0, N = blk.k0, blk.K, blk.n0, blk.N
    ks = slice(k0, k0 + K)
    want_inst = P.predict_xty(mode, K, N, False, blk.n_slab, rows // 32)
    y_eff = np.ascontiguousarray(W["y2"][:, n0 : n0 + N])
    t0, tail_d, tail_ld = 16, None, 0
    if blk.y_split:  # features [y_split, N) of the block come from a column block of another wide matrix
        y_eff[:, blk.y_split:] = W["tail"][:, t0 : t0 + N - blk.y_split]
        tail_d, tail_ld = _t(to_t32(P.poisoned(W["tail"], None, slice(t0, t0 + N - blk.y_split))), dev), NY
    x_d = _t(to_t32(P.poisoned(W["x"], None, ks)), dev)
    y_d = _t(to_t32(P.poisoned(W["y2"], None, slice(n0, n0 + (blk.y_split or N)))), dev)
    xc_d, yc_d = _t(to_t32(np.ascontiguousarray(W["x"][:, ks])), dev), _t(to_t32(y_eff), dev)
    used = K * N + (N if blk.want_bias else 0)
    slab = torch.full((blk.n_slab, used + 9), SENTINEL, device=dev)
    slab_c = torch.full((blk.n_slab, used), SENTINEL, device=dev)
    with _ctx(mode) as h:
        _ok(_xty(h, _p(x_d, 32 * k0), KX, _p(y_d, 32 * n0), NY, _p(tail_d, 32 * t0), blk.y_split, tail_ld, K, N, rows, blk.want_bias, 0.5,
                 slab, blk.n_slab), "xty block")
        assert _inst() == want_inst
        _ok(_xty(h, _p(xc_d), K, _p(yc_d), N, None, 0, 0, K, N, rows, blk.want_bias, 0.5, slab_c, blk.n_slab), "xty contiguous")
        assert _inst() == want_inst
    s = slab.cpu().numpy()
    assert (s[:, used:] == SENTINEL).all(), "a slab row is written behind K N (+ N)"
    assert (s[:, :used] != SENTINEL).all(), "every block writes its whole slab row"
    assert np.array_equal(_bits(s[:, :used]), _bits(slab_c.cpu().numpy())), "block == contiguous call, bit for bit"
    dw, db = P.xty_reference(W["x"][:, ks], y_eff, 0.5)
    tot = s[:, :used].astype(np.float64).sum(0)
    _close(tot[: K * N].reshape(K, N), dw, 1e-5, f"xty block dW {mode} {blk}")
    if blk.want_bias:
        _close(tot[K * N:], db, 1e-5, f"xty block db {mode} {blk}")


@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("K,N", [(70, 64), (5, 13), (155, 128)])
def test_dense_nonfinite_input_stays_in_its_row(dev, mode, K, N):
    """A NaN in the last feature of the last row of a tile - the element every clamped load past K repeats - reaches that row's
    outputs and no other's: the padding past K must read as zeros (zero weights do not help, 0 * NaN is NaN).  The f16x2
    kernel stages the clamped duplicates of its loads as zeros for this; the exact-f32 kernel clamps within the row."""
    rng = np.random.default_rng(K * 1000 + N)
    rows = 64
    x = rng.standard_normal((rows, K)).astype(np.float32)
    w = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    want = P.dense_reference(x, w, None, False, None)
    x[31, K - 1] = np.nan
    x_d, w_d = _t(to_t32(x), dev), _t(w, dev)
    y = _out(np.zeros(rows * N), dev)
    with _ctx(mode) as h:
        _ok(_dense(h, _p(x_d), K, _p(w_d), N, None, None, _p(y), N, K, N, rows, 0), "dense")
        assert _inst() == P.predict_dense(mode, K, N, False, False)
    got = from_t32(_main(y), rows, N)
    # the row that holds the NaN itself: NaN from the exact-f32 kernel.  The f16x2 epilogue's fmaxf(v, relu ? 0 : -FLT_MAX)
    # returns its other operand for a NaN and writes -FLT_MAX there: a known defect (support envelope of the
    # products), not asserted either way here - this test is about the OTHER rows
    if mode == "f32":
        assert np.isnan(got[31]).all(), "the row that holds the NaN"
    others = np.arange(rows) != 31
    _close(got[others], want[others], 1e-5, f"dense {mode} K={K} N={N}, rows without a NaN")


@pytest.mark.parametrize("mode", P.MODES)
def test_dense_chain_of_column_blocks(dev, mode):
    """GenericNet._dense's loop by hand: K = 900 in chunks of 384 with accumulate, N = 300 in blocks of 128."""
    rng = np.random.default_rng(900300)
    rows, K, N = 64, 900, 300
    x = rng.standard_normal((rows, K)).astype(np.float32)
    w = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    x_d, w_d, b_d = _t(to_t32(x), dev), _t(w, dev), _t(b, dev)
    y = _out(np.full(rows * N, np.nan), dev)
    with _ctx(mode) as h:
        for n0 in range(0, N, 128):
            nb = min(128, N - n0)
            for k0 in range(0, K, 384):
                kb = min(384, K - k0)
                _ok(_dense(h, _p(x_d, 32 * k0), K, _p(w_d, k0 * N + n0), N, _p(b_d, n0) if k0 == 0 else None, None, _p(y, 32 * n0), N, kb, nb,
                           rows, 0, int(k0 > 0)), "dense chain")
                assert _inst() == P.predict_dense(mode, kb, nb, False, k0 == 0)
    _close(from_t32(_main(y), rows, N), P.dense_reference(x, w, b, False, None), 1e-5, f"dense chain {mode}")


# ------------------------------------------------------------------------------------------ c. tiles per block
@pytest.mark.parametrize("c", P.WRAP_CASES, ids=P.case_id)
def test_dense_tiles_per_block(dev, c):
    d = P.wrap_data(c)
    K, N = c.K, c.N
    want_inst = P.wrap_instance(c)
    w_d, b_d = _t(d["w"], dev), _t(d["b"], dev)
    g_d = _t(to_t32(d["g"]), dev) if c.gate else None
    if c.rowmajor:
        x_d, idx_d = _t(d["src"], dev), _t(d["idx"], dev)
        gather = (_p(idx_d), d["Rm"], P.GATHER_E, P.GATHER_A, 1)
    else:
        x_d, gather = _t(to_t32(d["x"]), dev), None
    first = None
    with _ctx(c.mode) as h:
        for rows in P.WRAP_ROWS:  # a T32 matrix of fewer rows is a prefix of the large one
            y = _out(np.full(rows * N, np.nan), dev)
            _ok(_dense(h, _p(x_d), K, _p(w_d), N, _p(b_d), _p(g_d), _p(y), N, K, N, rows, 1, gather=gather), f"dense rows={rows}")
            assert _inst() == want_inst
            got = from_t32(_main(y), rows, N)
            _close(got, d["want"][:rows], 1e-5, f"dense {c} rows={rows}")
            if first is None:
                first = got.copy()
            assert np.array_equal(_bits(got[:32]), _bits(first)), f"rows=[0, 32) of the {rows}-row launch == the 32-row launch, bit for bit"


@pytest.mark.parametrize("mode", P.MODES)
def test_xty_tiles_per_block_and_blocks_without_a_tile(dev, mode):
    rng = np.random.default_rng(160)
    rows, (K, N) = P.XTY_TILE_ROWS, P.XTY_TILE_SHAPE
    x = rng.standard_normal((rows, K)).astype(np.float32)
    y = rng.standard_normal((rows, N)).astype(np.float32)
    dw, db = P.xty_reference(x, y, 0.25)
    x_d, y_d = _t(to_t32(x), dev), _t(to_t32(y), dev)
    used, tiles = K * N + N, rows // 32
    with _ctx(mode) as h:
        for n_slab in P.XTY_TILE_SLABS:
            slab = torch.full((n_slab, used + 3), SENTINEL, device=dev)
            _ok(_xty(h, _p(x_d), K, _p(y_d), N, None, 0, 0, K, N, rows, 1, 0.25, slab, n_slab), f"xty n_slab={n_slab}")
            want_inst = P.predict_xty(mode, K, N, False, n_slab, tiles)
            assert _inst() == want_inst
            if n_slab > tiles:
                assert want_inst == P.product_id(P.XTY, P.F32, P.T32, 3, 1), "more slabs than tiles: the exact-f32 kernel in either mode"
            s = slab.cpu().numpy()
            assert (s[:, used:] == SENTINEL).all()
            assert (s[tiles:, :used] == 0.0).all(), "a block without a tile writes zeros"
            assert (s[:tiles, :used] != SENTINEL).all()
            tot = s[:, :used].astype(np.float64).sum(0)
            _close(tot[: K * N].reshape(K, N), dw, 1e-5, f"xty dW {mode} n_slab={n_slab}")
            _close(tot[K * N:], db, 1e-5, f"xty db {mode} n_slab={n_slab}")


@pytest.mark.parametrize("share", [1, 3], ids=["own-rows", "shared-rows"])
def test_gather_wraps_past_2048_blocks(dev, share):
    from mava_amd._lib import lib, stream_ptr

    rng = np.random.default_rng(2049 + share)
    rows, K, KP, LD, A, Em, E = 32 * 2049, 3, 32, 5, 3, 32, 40
    Rm, T = Em * A, 32 * 2049 // (Em * A)
    src = rng.standard_normal((T * E * A // share, LD)).astype(np.float32)
    idx = rng.permutation(E)[:Em].astype(np.int32)
    src_d, idx_d = _t(src, dev), _t(idx, dev)
    for ids, ids_d in ((idx, idx_d), (None, None)):  # NULL: the identity, env = local env
        out = torch.full((rows * KP,), 7.0, device=dev)
        _ok(lib().mava_rec_gather_t32_f32(_p(src_d), _p(ids_d), Rm, E, A, share, LD, K, rows, KP, _p(out), stream_ptr()), "gather")
        got = from_t32(out.cpu().numpy(), rows, KP)
        want = src[P.gather_source_rows(rows, ids, Rm, E, A, share)][:, :K]
        assert np.array_equal(_bits(got[:, :K]), _bits(want)), "exact copies of the gathered rows"
        assert not got[:, K:].any(), "zeros past K"


def test_gather_widest_padding(dev):
    from mava_amd._lib import lib, stream_ptr

    rng = np.random.default_rng(1024)
    rows, K, KP, A, Em, E = 32, 700, 1024, 4, 8, 10
    src = rng.standard_normal((E * A, K)).astype(np.float32)
    idx = rng.permutation(E)[:Em].astype(np.int32)
    src_d, idx_d = _t(src, dev), _t(idx, dev)
    out = torch.full((rows * KP,), 7.0, device=dev)
    _ok(lib().mava_rec_gather_t32_f32(_p(src_d), _p(idx_d), Em * A, E, A, 1, K, K, rows, KP, _p(out), stream_ptr()), "gather 1024")
    got = from_t32(out.cpu().numpy(), rows, KP)
    assert np.array_equal(_bits(got[:, :K]), _bits(src[P.gather_source_rows(rows, idx, Em * A, E, A, 1)])) and not got[:, K:].any()


# ------------------------------------------------------------------------------------------ d. refusals launch nothing
def _refused(rc, arg, word, before, out, what):
    torch.cuda.synchronize()
    assert rc == -1000 - arg and rc <= -1000, f"{what}: return code {rc}, expected the argument error {-1000 - arg}"
    assert word in _last_error(), f"{what}: message {_last_error()!r} lacks {word!r}"
    assert _inst() == before, f"{what}: a refused launch leaves the diagnostic unchanged"
    assert (out.cpu().numpy() == SENTINEL).all(), f"{what}: a refused launch writes nothing"


@pytest.mark.parametrize("mode", P.MODES)
def test_dense_refusals_launch_nothing(dev, mode):
    rows = 64
    x_d = torch.ones(rows * 448, device=dev)
    w_d = torch.ones(448 * 384, device=dev)
    b_d = torch.ones(384, device=dev)
    idx_d = torch.zeros(4, dtype=torch.int32, device=dev)
    y = torch.full((rows * 384,), SENTINEL, device=dev)
    gather = (_p(idx_d), 16, 6, 4, 1)
    with _ctx(mode) as h:
        ok = torch.zeros(32 * 8, device=dev)
        _ok(_dense(h, _p(x_d), 8, _p(w_d), 8, None, None, _p(ok), 8, 8, 8, 32, 0), "a launch that runs")
        before = _inst()
        assert before == P.predict_dense(mode, 8, 8, False, False)
        for r in P.DENSE_REFUSALS:
            if r.mode != mode:
                continue
            assert P.predict_dense(mode, r.K, r.N, r.rowmajor, True) == Refusal(r.arg, r.word)
            rc = _dense(h, _p(x_d), r.K, _p(w_d), r.N, _p(b_d), None, _p(y), r.N, r.K, r.N, rows, 0, gather=gather if r.rowmajor else None)
            _refused(rc, r.arg, r.word, before, y, f"dense {r}")
        K, N = 70, 100
        for what, arg, word, kw in (("rows not a multiple of 32", 1, "multiple of 32", dict(rows=48)),
                                    ("x_ld < K", 5, "features per tile", dict(x_ld=K - 1)),
                                    ("row-major x_ld < K", 3, "gather", dict(x_ld=K - 1, gather=gather)),
                                    ("y_ld < N", 7, "y_ld", dict(y_ld=N - 1)),
                                    ("ldw < N", 0, "ldw", dict(ldw=N - 1))):
            a = dict(x_ld=K, ldw=N, y_ld=N, rows=rows, gather=None)
            a.update(kw)
            rc = _dense(h, _p(x_d), a["x_ld"], _p(w_d), a["ldw"], _p(b_d), None, _p(y), a["y_ld"], K, N, a["rows"], 0, gather=a["gather"])
            _refused(rc, arg, word, before, y, f"dense {what}")


@pytest.mark.parametrize("mode", P.MODES)
def test_xty_refusals_launch_nothing(dev, mode):
    rows = 96
    x_d = torch.ones(rows * 384, device=dev)
    y_d = torch.ones(rows * 384, device=dev)
    slab = torch.full((2, 384 * 384 // 2 + 384), SENTINEL, device=dev)
    with _ctx(mode) as h:
        ok = torch.zeros((1, 64 + 8), device=dev)
        _ok(_xty(h, _p(x_d), 8, _p(y_d), 8, None, 0, 0, 8, 8, 32, 1, 1.0, ok, 1), "a launch that runs")
        before = _inst()
        assert before == P.predict_xty(mode, 8, 8, False, 1, 1)
        for r in P.XTY_REFUSALS:
            if r.mode != mode:
                continue
            assert r.K * r.N + r.N <= slab.shape[1]
            rc = _xty(h, _p(x_d), r.K, _p(y_d), r.N, None, 0, 0, r.K, r.N, rows, 1, 1.0, slab, 2)
            _refused(rc, r.arg, r.word, before, slab, f"xty {r}")
        K, N = 70, 128
        for what, arg, word, kw in (("rows not a multiple of 32", 1, "rows", dict(rows=48)),
                                    ("no slab", 1, "n_slab", dict(n_slab=0)),
                                    ("x_ld < K", 5, "x_ld", dict(x_ld=K - 1)),
                                    ("y_ld < N", 6, "y_ld", dict(y_ld=N - 1)),
                                    ("slab_stride too small", 2, "slab_stride", dict(slab_stride=K * N + N - 1)),
                                    ("y_split not a multiple of 32", 10, "y_split", dict(y_tail=_p(y_d), y_split=40, y_tail_ld=N - 40)),
                                    ("y_tail narrower than N - y_split", 10, "y_tail", dict(y_tail=_p(y_d), y_split=32, y_tail_ld=N - 33))):
            a = dict(x_ld=K, y_ld=N, rows=rows, n_slab=2, slab_stride=None, y_tail=None, y_split=0, y_tail_ld=0)
            a.update(kw)
            rc = _xty(h, _p(x_d), a["x_ld"], _p(y_d), a["y_ld"], a["y_tail"], a["y_split"], a["y_tail_ld"], K, N, a["rows"], 1, 1.0, slab,
                      a["n_slab"], slab_stride=a["slab_stride"])
            _refused(rc, arg, word, before, slab, f"xty {what}")
