"""CPU: the case tables of tests/product_instances.py reach, through its restatement of the dispatch, EVERY dense and X^T Y
template instance the host dispatchers name (csrc/rec_dense.hip, rec_dense_h2.hip) - the lists below are written out from the
dispatchers, not derived from the tables - every fall-through from the f16x2 arithmetic to the exact-f32 kernels, and every
refusal.  The dispatch lists of the sources are read back, so a line added there without a case here fails."""
import os
import re

import numpy as np

from tests import product_instances as P
from tests.product_instances import DENSE, F32, FULLK, H2, LEAN, ROWMAJOR, T32, XTY, Refusal, product_id

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mava_amd", "csrc")

# --- rec_dense.hip, DENSE_CASE -> launch_dense<NB, NTW>: FULLK for all, clamped and row-major forms for NTW = 1 only
_DENSE_F32 = [(2, 1), (4, 1), (6, 1), (8, 1), (12, 1), (18, 1), (24, 1), (8, 2), (12, 2), (8, 3)]
DENSE_F32_IDS = ({product_id(DENSE, F32, FULLK, nb, ntw) for nb, ntw in _DENSE_F32}
                 | {product_id(DENSE, F32, form, nb, 1) for nb, ntw in _DENSE_F32 if ntw == 1 for form in (T32, ROWMAJOR)})
# --- rec_dense_h2.hip, DENSE_H2 and the LEAN K = 384 form
_DENSE_H2 = [(1, 1), (2, 1), (4, 1), (6, 1), (8, 1), (10, 1), (12, 1), (18, 1), (8, 3)]
DENSE_H2_IDS = {product_id(DENSE, H2, T32, nb, ntw) for nb, ntw in _DENSE_H2} | {product_id(DENSE, H2, LEAN, 24, 1)}
# --- rec_dense.hip, XTY_CASE (one kernel reads T32 and row-major x) and rec_dense_h2.hip, XTY_H2
_XTY_F32 = [(1, 1), (2, 1), (3, 1), (4, 1), (6, 1), (9, 1), (12, 1), (4, 2), (6, 2), (4, 3)]
_XTY_H2 = [(3, 1), (4, 1), (5, 1), (6, 1), (9, 1), (4, 3)]
XTY_F32_IDS = {product_id(XTY, F32, T32, kt, ntw) for kt, ntw in _XTY_F32}
XTY_H2_IDS = {product_id(XTY, H2, T32, kt, ntw) for kt, ntw in _XTY_H2}


def _dense_ids(mode):
    return {P.predict_dense(m, c.K, c.N, c.rowmajor, c.bias) for m, c in P.dense_runs() if m == mode}


def _xty_ids(mode):
    return {P.predict_xty(m, c.K, c.N, c.rowmajor, c.n_slab, c.rows // 32) for m, c in P.xty_runs() if m == mode}


def test_instance_ids_are_distinct():
    ids = DENSE_F32_IDS | DENSE_H2_IDS | XTY_F32_IDS | XTY_H2_IDS | {product_id(XTY, F32, ROWMAJOR, kt, ntw) for kt, ntw in _XTY_F32}
    assert len(ids) == 24 + 10 + 10 + 6 + 10
    assert product_id(DENSE, H2, LEAN, 24, 1) == 1230241 and product_id(XTY, F32, T32, 4, 3) == 2100043


def test_the_sources_name_exactly_these_instances():
    with open(os.path.join(CSRC, "rec_dense.hip")) as f:
        f32_src = f.read()
    with open(os.path.join(CSRC, "rec_dense_h2.hip")) as f:
        h2_src = f.read()
    pairs = lambda macro, src: [(int(a), int(b)) for a, b in re.findall(macro + r"\((\d+), (\d+)\)", src)]
    assert pairs("DENSE_CASE", f32_src) == _DENSE_F32 == list(P.DENSE_CASE)
    assert pairs("XTY_CASE", f32_src) == _XTY_F32 == list(P.XTY_CASE)
    assert pairs("DENSE_H2", h2_src) == _DENSE_H2 == list(P.DENSE_H2)
    assert pairs("XTY_H2", h2_src) == _XTY_H2 == list(P.XTY_H2)
    assert re.findall(r"launch_dense_h2<(\d+), (\d+), true>", h2_src) == [("24", "1")]  # the one LEAN instance


def test_dense_tables_reach_every_instance():
    f32, h2 = _dense_ids("f32"), _dense_ids("f16x2")
    assert not any(isinstance(i, Refusal) for i in f32 | h2), "a case that runs is not a refusal"
    assert f32 == DENSE_F32_IDS
    assert {i for i in h2 if i // 100000 % 10 == H2} == DENSE_H2_IDS
    # what the f16x2 mode hands to the exact-f32 kernels: row-major input (all seven instances), N in 129..256 (both FULLK
    # instances of two tiles per wave), 19..24 batches with a bias
    fall = {i for i in h2 if i // 100000 % 10 == F32}
    assert {product_id(DENSE, F32, ROWMAJOR, nb, 1) for nb, ntw in _DENSE_F32 if ntw == 1} <= fall
    assert {product_id(DENSE, F32, FULLK, 8, 2), product_id(DENSE, F32, FULLK, 12, 2)} <= fall
    assert {product_id(DENSE, F32, FULLK, 24, 1), product_id(DENSE, F32, T32, 24, 1)} <= fall
    assert any(c.K == 384 and c.N <= 128 and c.bias for c in P.DENSE_CASES) and any(c.K == 384 and not c.bias for c in P.DENSE_CASES)


def test_dense_cases_cover_the_edges():
    C = P.DENSE_CASES + P.DENSE_H2_ONLY_CASES
    assert any(c.K == 1 for c in C)
    for N in (13, 100, 130, 300):  # a ragged last 32-feature tile
        assert any(c.N == N for c in C), N
    for NB in (1, 2, 4, 6, 8, 10, 12, 18, 24):
        for K in (16 * NB, 16 * NB - 1, 16 * (NB - 1) + 1):
            assert any(c.K == K and not c.rowmajor for c in C), K
    t32 = [c for c in C if not c.rowmajor]
    for bias, relu, gate in ((True, False, False), (False, False, False), (False, True, False), (False, False, True), (True, True, True)):
        assert any((c.bias, c.relu, c.gate) == (bias, relu, gate) for c in t32), (bias, relu, gate)
    assert all(c.rows % 32 == 0 and 32 <= c.rows <= 128 for c in C)
    assert len(set(C)) == len(C)


def test_xty_tables_reach_every_instance():
    f32, h2 = _xty_ids("f32"), _xty_ids("f16x2")
    assert not any(isinstance(i, Refusal) for i in f32 | h2)
    assert {i for i in f32 if i // 10000 % 10 == T32} == XTY_F32_IDS
    assert {i for i in f32 if i // 10000 % 10 == ROWMAJOR} >= {product_id(XTY, F32, ROWMAJOR, 3, 1), product_id(XTY, F32, ROWMAJOR, 4, 3)}
    assert {i for i in h2 if i // 100000 % 10 == H2} == XTY_H2_IDS
    fall = {i for i in h2 if i // 100000 % 10 == F32}
    assert product_id(XTY, F32, T32, 12, 1) in fall                                         # kt in 10..12
    assert {product_id(XTY, F32, T32, 4, 2), product_id(XTY, F32, T32, 6, 2)} <= fall       # N in 129..256
    assert product_id(XTY, F32, ROWMAJOR, 3, 1) in fall                                     # row-major x
    # more slabs than tiles: a shape the f16x2 kernel takes otherwise
    over = [c for c in P.XTY_CASES if c.n_slab > c.rows // 32 and not c.rowmajor]
    assert over and all(P.predict_xty("f16x2", c.K, c.N, False, c.rows // 32, c.rows // 32) // 100000 % 10 == H2 for c in over)
    assert all(P.predict_xty("f16x2", c.K, c.N, False, c.n_slab, c.rows // 32) // 100000 % 10 == F32 for c in over)
    C = P.XTY_CASES
    assert {c.want_bias for c in C} == {0, 1} and any(c.scale != 1.0 for c in C)
    assert any(c.y_split == 32 for c in C) and any(c.y_split and c.y_split == (c.N - 1) // 32 * 32 and c.y_split > 32 for c in C)
    assert all(c.y_split % 32 == 0 and c.y_split < c.N for c in C)


def test_refusals_and_the_asymmetry_above_256_outputs():
    for r in P.DENSE_REFUSALS:
        for bias in (False, True):
            assert P.predict_dense(r.mode, r.K, r.N, r.rowmajor, bias) == Refusal(r.arg, r.word), r
    for r in P.XTY_REFUSALS:
        assert P.predict_xty(r.mode, r.K, r.N, False, 2, 3) == Refusal(r.arg, r.word), r
    got = {(r.mode, r.K, r.N, r.rowmajor, r.arg) for r in P.DENSE_REFUSALS}
    for m in P.MODES:
        assert (m, 384, 129, False, 4) in got and (m, 130, 256, False, 9) in got and (m, 70, 130, True, 9) in got
        assert any(r.mode == m and (r.K, r.N, r.arg) == (224, 256, 4) for r in P.XTY_REFUSALS)
    # K = 100 with N = 384: f16x2 <8,3> takes any K <= 128, the exact-f32 <8,3> is FULLK only
    assert P.DenseCase(100, 384, True, True, True) in P.DENSE_H2_ONLY_CASES
    assert P.predict_dense("f16x2", 100, 384, False, True) == product_id(DENSE, H2, T32, 8, 3)
    assert P.predict_dense("f32", 100, 384, False, True) == Refusal(9, "not instantiated")
    assert P.predict_dense("f32", 128, 384, False, True) == product_id(DENSE, F32, FULLK, 8, 3)


def test_support_envelope_of_the_exact_f32_dense_kernel():
    """What the refusal message of launch_dense and DESIGN.md state: T32 inputs of ANY width run with N <= 128 (the clamped
    form reads x_ld at run time, padded inputs included), K = 128 or 192 with N <= 256, K = 128 with N <= 384."""
    for K in range(1, 385):
        for N in (1, 128, 129, 256, 257, 384):
            runs = not isinstance(P.predict_dense("f32", K, N, False, True), Refusal)
            assert runs == (N <= 128 or (K in (128, 192) and N <= 256) or K == 128), (K, N)
            h2 = not isinstance(P.predict_dense("f16x2", K, N, False, True), Refusal)
            assert h2 == (runs or (K <= 128 and N >= 257)), (K, N)
            rm = not isinstance(P.predict_dense("f16x2", K, N, True, True), Refusal)
            assert rm == (N <= 128)
    for K in range(1, 385):
        for N in (1, 128, 129, 256, 257, 384):
            kt, ntw = (K + 31) // 32, P._ntw(N)
            for m in P.MODES:
                assert (not isinstance(P.predict_xty(m, K, N, False, 2, 3), Refusal)) == (kt * ntw <= 12)


def test_wrap_and_block_tables():
    assert {P.wrap_instance(c) for c in P.WRAP_CASES} == P.WRAP_INSTANCES
    assert any(c.gate for c in P.WRAP_CASES if P.wrap_instance(c) == product_id(DENSE, F32, T32, 2, 1))
    assert any(not c.gate for c in P.WRAP_CASES if P.wrap_instance(c) == product_id(DENSE, F32, T32, 2, 1))
    assert P.WRAP_ROWS == (32, 64, 32 * 257, 32 * (4 * 256 + 1))
    for b in P.DENSE_BLOCKS + P.XTY_BLOCKS:
        assert b.k0 + b.K <= P.WIDE_K and b.n0 + b.N <= P.WIDE_N, b
    have = {(b.k0, b.K, b.n0, b.N, b.accumulate) for b in P.DENSE_BLOCKS}
    assert {(0, 384, 0, 128, 0), (384, 64, 128, 128, 1), (32, 70, 256, 64, 0), (0, 16, 288, 13, 0)} <= have
    # gated products whose last wave has lanes without a feature (N mod 32 in 1..4): contiguous, in both prefetch paths and
    # the LEAN form, and as blocks that end at the last column of the wide matrix
    edge = [c for c in P.DENSE_CASES if c.gate and 1 <= c.N % 32 <= 4]
    assert {c.N for c in edge} >= {1, 2, 4, 33, 65, 97, 100} and all(c.rows * c.N * 4 % 512 == 0 for c in edge if c.rows == 128)
    assert any(c.K <= 32 for c in edge) and any(c.K > 288 and not c.bias for c in edge)
    assert any(b.gate and 1 <= b.N % 32 <= 4 and b.n0 + b.N == P.WIDE_N for b in P.DENSE_BLOCKS)


def test_references_and_t32_round_trip():
    c = P.DenseCase(5, 13, True, True, True)
    d = P.dense_data(c)
    want = np.maximum(d["x"].astype(np.float64) @ d["w"].astype(np.float64) + d["b"], 0) * (d["g"] > 0)
    assert np.array_equal(d["want"], want) and want.dtype == np.float64
    a = np.arange(64 * 3, dtype=np.float32).reshape(64, 3)
    assert np.array_equal(P.from_t32(P.to_t32(a), 64, 3), a) and P.to_t32(a)[32] == a[0, 1]
    # the gather of a row-major case: time-major rows, env ids through idx
    r = P.dense_data(P.DenseCase(20, 100, True, True, False, True))
    T = r["x"].shape[0] // r["Rm"]
    src = r["src"].reshape(T, P.GATHER_E, P.GATHER_A, 20)
    assert np.array_equal(r["x"], src[:, r["idx"]].reshape(-1, 20))
    dw, db = P.xty_reference(np.ones((32, 2)), np.full((32, 3), 2.0), 0.5)
    assert np.array_equal(dw, np.full((2, 3), 32.0)) and np.array_equal(db, np.full(3, 32.0))
    p = P.poisoned(np.ones((4, 4), np.float32), slice(1, 3), slice(0, 2))
    assert np.isnan(p).sum() == 12 and p[1, 0] == 1.0
