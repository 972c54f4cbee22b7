"""Case tables of tests/test_gpu_products.py and a Python restatement of the host dispatch of the dense and X^T Y products
(csrc/rec_dense.hip: mava_rec_dense_f32, mava_rec_xty_f32, launch_dense; csrc/rec_dense_h2.hip: mava_rec_dense_h2_launch,
mava_rec_xty_h2_launch): which template instance a shape must reach, as the integer mava_debug_rec_product_last_instance()
reports (rec_task.h: rec_product_instance_id; DESIGN.md §"No process-wide state"), or which argument error refuses it.  Plain
NumPy and float64 only: tests/test_product_instances_table.py checks the tables without a GPU."""
from functools import lru_cache
from typing import NamedTuple, Union

import numpy as np

from tests.seq_model import from_t32, to_t32  # noqa: F401  (re-exported for the GPU tests)

DENSE, XTY = 1, 2          # operation
F32, H2 = 1, 2             # family: exact-f32 MFMAs | split-f16 operands
T32, FULLK, ROWMAJOR, LEAN = 0, 1, 2, 3  # form (dense f32: T32 = the clamped-address form)
MODES = ("f32", "f16x2")


def product_id(op, family, form, p, ntw):
    """rec_task.h rec_product_instance_id; p = NB (dense) or KT (xty)."""
    return op * 1000000 + family * 100000 + form * 10000 + p * 10 + ntw


class Refusal(NamedTuple):
    arg: int   # the entry point returns -1000 - arg
    word: str  # a piece of the error message


# the four dispatch lists, in the order the dispatchers test them
DENSE_CASE = ((2, 1), (4, 1), (6, 1), (8, 1), (12, 1), (18, 1), (24, 1), (8, 2), (12, 2), (8, 3))
DENSE_H2 = ((1, 1), (2, 1), (4, 1), (6, 1), (8, 1), (10, 1), (12, 1), (18, 1), (8, 3))  # then LEAN <24, 1> without a bias
XTY_CASE = ((1, 1), (2, 1), (3, 1), (4, 1), (6, 1), (9, 1), (12, 1), (4, 2), (6, 2), (4, 3))
XTY_H2 = ((3, 1), (4, 1), (5, 1), (6, 1), (9, 1), (4, 3))


def _ntw(N):
    return ((N + 31) // 32 + 3) // 4  # 32-feature output tiles per wave: 1 up to N = 128, 2 up to 256, 3 up to 384


def predict_dense(mode, K, N, rowmajor, has_bias) -> Union[int, Refusal]:
    """mava_rec_dense_f32 with valid pointers, leading dimensions and row count."""
    if not (1 <= K <= 384 and 1 <= N <= 384):
        return Refusal(0, "unsupported")
    nb, ntw = (K + 15) // 16, _ntw(N)
    if mode == "f16x2" and not rowmajor:  # mava_rec_dense_h2_launch: anything it does not take falls through to exact f32
        for NB, NTW in DENSE_H2:
            if nb <= NB and ntw == NTW:
                return product_id(DENSE, H2, T32, NB, NTW)
        if nb <= 24 and ntw == 1 and not has_bias:
            return product_id(DENSE, H2, LEAN, 24, 1)
    if nb * ntw * 8 > 192:
        return Refusal(4, "weight slice")
    for NB, NTW in DENSE_CASE:
        if nb <= NB and ntw == NTW:  # launch_dense<NB, NTW>
            if rowmajor:
                return product_id(DENSE, F32, ROWMAJOR, NB, 1) if NTW == 1 else Refusal(9, "row-major")
            if K == 16 * NB:
                return product_id(DENSE, F32, FULLK, NB, NTW)
            return product_id(DENSE, F32, T32, NB, 1) if NTW == 1 else Refusal(9, "not instantiated")
    return Refusal(9, "not instantiated")  # (unreachable: the list covers every nb * ntw <= 24)


def predict_xty(mode, K, N, rowmajor, n_slab, tiles) -> Union[int, Refusal]:
    """mava_rec_xty_f32 with valid pointers, leading dimensions, slab stride; tiles = rows / 32."""
    if not (1 <= K <= 384 and 1 <= N <= 384):
        return Refusal(0, "unsupported")
    if not (tiles >= 1 and 1 <= n_slab <= 1024):
        return Refusal(1, "n_slab")
    kt, ntw = (K + 31) // 32, _ntw(N)
    if mode == "f16x2" and not rowmajor:
        for KT, NTW in XTY_H2:
            if kt <= KT and ntw == NTW:
                if n_slab > tiles:  # launch_xty_h2: every block must own a tile
                    break
                return product_id(XTY, H2, T32, KT, NTW)
    if kt * ntw > 12:
        return Refusal(4, "accumulator tiles")
    for KT, NTW in XTY_CASE:
        if kt <= KT and ntw == NTW:
            return product_id(XTY, F32, ROWMAJOR if rowmajor else T32, KT, NTW)
    return Refusal(9, "not instantiated")  # (unreachable)


# ------------------------------------------------------------------------------------------- case tables
class DenseCase(NamedTuple):
    K: int
    N: int
    bias: bool = True
    relu: bool = False
    gate: bool = False
    rowmajor: bool = False
    rows: int = 64


def _dense_cases():
    D = DenseCase
    c = []
    # K at 16 NB exactly (exact f32: the FULLK form), at 16 NB - 1 and at 16 (NB - 1) + 1 (clamped form) of every NTW = 1
    # instance of either family, N over full and ragged last tiles, the epilogue's options in turn
    opts = ((True, False, False), (False, True, False), (True, False, True), (False, True, True), (True, True, False), (False, False, False))
    widths = (128, 13, 100, 32, 96, 64, 127, 33)
    i = 0
    for NB in (1, 2, 4, 6, 8, 10, 12, 18, 24):
        for K in (16 * NB, 16 * NB - 1, 16 * (NB - 1) + 1):
            b, r, g = opts[i % len(opts)]
            c.append(D(K, widths[i % len(widths)], b, r, g))
            i += 1
    c += [D(384, 128, False, True, True), D(369, 100, False, False, False), D(300, 13, False, True, False)]  # LEAN: no bias
    c += [D(384, 128, True, False, True), D(289, 100, True, True, False)]  # the LEAN shape with a bias: exact f32 <24,1>
    # wider than 128 outputs.  Exact f32: FULLK only (K = 128 / 192 up to 256, K = 128 up to 384); f16x2: <8,3> for any K <= 128
    # with N in 257..384, N in 129..256 falls through to exact f32
    c += [D(128, 130, True, True, False), D(128, 256, False, False, True), D(192, 130, True, False, True), D(192, 200, False, True, False),
          D(128, 300, True, True, True), D(128, 384, False, False, False), D(128, 257, True, False, False)]
    # a gate with N mod 32 in 1..4: the upper half of wave N / 32 has no feature of its own (32 w + 4 >= N), and its prefetched
    # gate loads must fall back to feature 32 w, not to their own first feature behind the block.  128 rows make the gate
    # matrix a multiple of 512 bytes, so it ends where its allocation ends.  (A read leaves no trace a test can assert on:
    # these shapes are here for the result and so that a run under a memory checker meets them.)
    c += [D(20, 33, True, False, True, False, 128), D(70, 65, False, True, True, False, 128), D(128, 97, True, False, True, False, 128),
          D(200, 100, True, True, True, False, 128), D(50, 1, True, False, True, False, 128), D(24, 2, False, False, True, False, 128),
          D(300, 4, False, True, True, False, 128)]
    # row-major gathered input: exact f32 in either mode
    c += [D(K, N, b, r, False, True) for K, N, b, r in ((20, 100, True, True), (50, 128, False, False), (70, 13, True, False),
                                                        (120, 96, True, True), (155, 128, True, False), (200, 64, False, True),
                                                        (300, 128, True, True))]
    return c


DENSE_CASES = _dense_cases()
# runs in f16x2 mode on <8,3>, refused in exact-f32 mode (no clamped form above 128 outputs): the asymmetry the code has today
DENSE_H2_ONLY_CASES = [DenseCase(100, 384, True, True, True), DenseCase(1, 300, False, False, False), DenseCase(113, 257, True, False, True)]


class DenseRefusal(NamedTuple):
    mode: str
    K: int
    N: int
    rowmajor: bool
    arg: int
    word: str


DENSE_REFUSALS = (
    [DenseRefusal(m, 384, 129, False, 4, "weight slice") for m in MODES]
    + [DenseRefusal(m, 208, 200, False, 4, "weight slice") for m in MODES]   # nb = 13, two tiles per wave: 208 registers
    + [DenseRefusal(m, 144, 300, False, 4, "weight slice") for m in MODES]   # nb = 9, three tiles per wave (f16x2 <8,3> ends at 128)
    + [DenseRefusal(m, 130, 256, False, 9, "not instantiated") for m in MODES]
    + [DenseRefusal(m, 70, 130, True, 9, "row-major") for m in MODES]
    + [DenseRefusal("f32", c.K, c.N, False, 9, "not instantiated") for c in DENSE_H2_ONLY_CASES]
)


class XtyCase(NamedTuple):
    K: int
    N: int
    want_bias: int = 1
    scale: float = 1.0
    y_split: int = 0     # > 0: features [y_split, N) come from y_tail
    n_slab: int = 2
    rowmajor: bool = False
    rows: int = 96       # three tiles


def _xty_cases():
    X = XtyCase
    c = [X(20, 13), X(32, 100, 0, 0.5), X(50, 128, 1, 0.25), X(64, 64, 0), X(70, 100, 1, 2.0), X(96, 128, 0, 1.0, 32),
         X(100, 96, 1, 0.5, 64), X(128, 128, 1, 1.0, 96), X(150, 64, 0, 0.125), X(160, 100, 1), X(180, 128, 1, 4.0, 32),
         X(250, 40, 1, 0.5), X(288, 128, 0), X(300, 128, 1, 0.25), X(384, 32, 1), X(350, 13, 0, 2.0),
         X(100, 200, 1, 0.5), X(128, 256, 0, 1.0, 224), X(160, 130, 1, 0.25, 128), X(192, 256, 1),
         X(128, 384, 1, 0.25, 352), X(37, 300, 0, 1.0, 288), X(1, 257, 1, 2.0, 32)]
    c += [X(70, 128, 1, 1.0, 0, 5), X(128, 384, 1, 0.5, 0, 4)]  # more slabs than tiles: exact f32 in either mode
    c += [X(70, 128, 1, 0.5, 0, 2, True), X(20, 300, 0, 1.0, 0, 3, True)]  # row-major gathered x
    return c


XTY_CASES = _xty_cases()


class XtyRefusal(NamedTuple):
    mode: str
    K: int
    N: int
    arg: int
    word: str


XTY_REFUSALS = ([XtyRefusal(m, 224, 256, 4, "accumulator tiles") for m in MODES]
                + [XtyRefusal(m, 160, 300, 4, "accumulator tiles") for m in MODES])


def case_id(c):
    return "-".join(str(int(v)) if isinstance(v, bool) else str(v) for v in c)


def dense_runs():
    """(mode, case) of every dense case in every mode that runs it."""
    return [(m, c) for c in DENSE_CASES for m in MODES] + [("f16x2", c) for c in DENSE_H2_ONLY_CASES]


def xty_runs():
    return [(m, c) for c in XTY_CASES for m in MODES]


# ---- row-major gather (rec_task.h gather_row): batch row q -> t = q / Rm, m = q % Rm, env = idx[m / A], agent = m % A
GATHER_E, GATHER_A, GATHER_EM = 6, 4, 4  # Rm = 16 rows per step


def gather_source_rows(rows, idx, Rm, E, A, share):
    q = np.arange(rows)
    t, m = q // Rm, q % Rm
    e_local, a = m // A, m % A
    env = e_local if idx is None else np.asarray(idx)[e_local]
    return ((t * E + env) * A + a) // share


# ------------------------------------------------------------------------------------------ float64 references
def dense_reference(x, w, b, relu, gate, y_old=None):
    """act(x @ w + b) * (gate > 0) (+ y_old enters before the activation: the kernel starts its accumulators from it)."""
    y = np.asarray(x, np.float64) @ np.asarray(w, np.float64)
    if b is not None:
        y = y + np.asarray(b, np.float64)
    if y_old is not None:
        y = y + np.asarray(y_old, np.float64)
    if relu:
        y = np.maximum(y, 0.0)
    if gate is not None:
        y = y * (np.asarray(gate) > 0)
    return y


def xty_reference(x, y, scale):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return scale * (x.T @ y), scale * y.sum(0)


def _seed(c):
    return [int(round(abs(float(v)) * 8)) for v in c]


@lru_cache(maxsize=None)
def dense_data(c: DenseCase):
    """Inputs of one dense case (standard-normal x, W scaled by 1 / sqrt(K)) and its float64 result.  Row-major cases carry the
    external (T, E, A, K) source, the env ids of the minibatch and the gathered rows."""
    rng = np.random.default_rng([6] + _seed(c))
    K, N, rows = c.K, c.N, c.rows
    d = {}
    if c.rowmajor:
        Rm = GATHER_EM * GATHER_A
        src = rng.standard_normal((rows // Rm * GATHER_E * GATHER_A, K)).astype(np.float32)
        idx = rng.permutation(GATHER_E)[:GATHER_EM].astype(np.int32)
        x = src[gather_source_rows(rows, idx, Rm, GATHER_E, GATHER_A, 1)]
        d.update(src=src, idx=idx, Rm=Rm)
    else:
        x = rng.standard_normal((rows, K)).astype(np.float32)
    w = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32) if c.bias else None
    g = rng.standard_normal((rows, N)).astype(np.float32) if c.gate else None
    d.update(x=x, w=w, b=b, g=g, want=dense_reference(x, w, b, c.relu, g))
    return d


@lru_cache(maxsize=None)
def xty_data(c: XtyCase):
    rng = np.random.default_rng([7] + _seed(c))
    K, N, rows = c.K, c.N, c.rows
    d = {}
    if c.rowmajor:
        Rm = GATHER_EM * GATHER_A
        src = rng.standard_normal((rows // Rm * GATHER_E * GATHER_A, K)).astype(np.float32)
        idx = rng.permutation(GATHER_E)[:GATHER_EM].astype(np.int32)
        x = src[gather_source_rows(rows, idx, Rm, GATHER_E, GATHER_A, 1)]
        d.update(src=src, idx=idx, Rm=Rm)
    else:
        x = rng.standard_normal((rows, K)).astype(np.float32)
    y = rng.standard_normal((rows, N)).astype(np.float32)
    dw, db = xty_reference(x, y, c.scale)
    d.update(x=x, y=y, dw=dw, db=db)
    return d


# ---- column blocks of one wide problem (GenericNet._dense / _xty: x advanced by 32 k0 floats with x_ld > K, a W block with
# ldw > N, y and gate advanced by 32 n0 floats with y_ld > N)
WIDE_K, WIDE_N, WIDE_ROWS = 448, 320, 64


class Block(NamedTuple):
    k0: int
    K: int
    n0: int
    N: int
    accumulate: int = 0
    bias: bool = True
    relu: bool = False
    gate: bool = False


DENSE_BLOCKS = [Block(0, 384, 0, 128, 0, False, False, False), Block(384, 64, 128, 128, 1, False, True, True), Block(32, 70, 256, 64, 0, True, True, True),
                Block(0, 16, 288, 13, 0, True, False, True), Block(64, 384, 192, 128, 1, True, False, False), Block(5 * 32, 155, 32, 100, 1, True, True, False),
                Block(96, 128, 0, 320, 0, True, False, True), Block(0, 192, 64, 256, 1, False, True, False), Block(447, 1, 319, 1, 0, True, False, True), Block(10, 50, 223, 97, 1, False, True, True)]


class XtyBlock(NamedTuple):
    k0: int
    K: int
    n0: int
    N: int
    want_bias: int = 1
    y_split: int = 0
    n_slab: int = 2


XTY_BLOCKS = [XtyBlock(0, 128, 0, 128), XtyBlock(128, 128, 128, 128, 0), XtyBlock(32, 70, 256, 64), XtyBlock(384, 64, 192, 100, 1, 32),
              XtyBlock(96, 300, 0, 128, 1, 0, 3), XtyBlock(0, 128, 0, 320, 1, 288), XtyBlock(447, 1, 307, 13, 1), XtyBlock(200, 150, 64, 256, 0, 128)]


@lru_cache(maxsize=None)
def wide_data():
    rng = np.random.default_rng(448320)
    x = rng.standard_normal((WIDE_ROWS, WIDE_K)).astype(np.float32)
    w = (rng.standard_normal((WIDE_K, WIDE_N)) / np.sqrt(WIDE_K)).astype(np.float32)
    b = rng.standard_normal(WIDE_N).astype(np.float32)
    g = rng.standard_normal((WIDE_ROWS, WIDE_N)).astype(np.float32)
    y_old = rng.standard_normal((WIDE_ROWS, WIDE_N)).astype(np.float32)
    y2 = rng.standard_normal((WIDE_ROWS, WIDE_N)).astype(np.float32)  # the Y operand of the X^T Y blocks
    tail = rng.standard_normal((WIDE_ROWS, WIDE_N)).astype(np.float32)
    return dict(x=x, w=w, b=b, g=g, y_old=y_old, y2=y2, tail=tail)


def poisoned(a, rows=None, cols=None):
    """A float32 copy of the 2-D array `a` with NaN everywhere outside rows x cols (slices; None = all)."""
    out = np.full(a.shape, np.nan, np.float32)
    r, c = rows if rows is not None else slice(None), cols if cols is not None else slice(None)
    out[r, c] = a[r, c]
    return out


# ---- tiles per block: dense launches are capped at 256 blocks; 32 * 257 rows give block 0 two tiles, 32 * (4 * 256 + 1) five
# (the PF = 3 prologue of the NB <= 2 path is used up after three), 32 and 64 rows one tile per block
WRAP_ROWS = (32, 64, 32 * 257, 32 * (4 * 256 + 1))


class WrapCase(NamedTuple):
    mode: str
    K: int
    N: int
    gate: bool = False
    rowmajor: bool = False


# (exact f32 <8,1> FULLK exists at K = 128 only: its x matrix is 16.8 MB at the largest row count, the row-major source of
# <6,1> 13.8 MB - above the 10 MB the other cases keep to, there is no smaller shape that reaches those instances)
WRAP_CASES = [WrapCase("f32", 24, 20), WrapCase("f32", 24, 20, True), WrapCase("f32", 50, 32, True), WrapCase("f32", 128, 32, True),
              WrapCase("f32", 70, 32, False, True), WrapCase("f16x2", 70, 32, False, True), WrapCase("f16x2", 10, 32, True),
              WrapCase("f16x2", 50, 20, True)]
WRAP_INSTANCES = {product_id(DENSE, F32, T32, 2, 1), product_id(DENSE, F32, T32, 4, 1), product_id(DENSE, F32, FULLK, 8, 1),
                  product_id(DENSE, F32, ROWMAJOR, 6, 1), product_id(DENSE, H2, T32, 1, 1), product_id(DENSE, H2, T32, 4, 1)}


def wrap_instance(c: WrapCase):
    return predict_dense(c.mode, c.K, c.N, c.rowmajor, True)


@lru_cache(maxsize=2)
def wrap_data(c: WrapCase):
    """One draw at the largest row count; the smaller launches read its first rows (a T32 matrix of fewer rows is a prefix)."""
    rng = np.random.default_rng([8] + _seed(c[1:]))
    rows, K, N = WRAP_ROWS[-1], c.K, c.N
    d = {}
    if c.rowmajor:
        Rm = GATHER_EM * GATHER_A
        src = rng.standard_normal((rows // Rm * GATHER_E * GATHER_A, K)).astype(np.float32)
        idx = rng.permutation(GATHER_E)[:GATHER_EM].astype(np.int32)
        x = src[gather_source_rows(rows, idx, Rm, GATHER_E, GATHER_A, 1)]
        d.update(src=src, idx=idx, Rm=Rm)
    else:
        x = rng.standard_normal((rows, K)).astype(np.float32)
    w = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    g = rng.standard_normal((rows, N)).astype(np.float32) if c.gate else None
    d.update(x=x, w=w, b=b, g=g, want=dense_reference(x, w, b, True, g))
    return d


XTY_TILE_ROWS = 160                      # five tiles
XTY_TILE_SLABS = (1, 2, 3, 5, 8)         # tiles per block 5 | 3,2 | 2,2,1 | 1 each | three blocks without a tile
XTY_TILE_SHAPE = (70, 100)               # exact f32 <3,1>, f16x2 <3,1>
