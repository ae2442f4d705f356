"""The training GEMMs of csrc/gemm.hip called directly, on inputs whose result is EXACT (tests/gemm_reference.py): integer
operands for all five entry points, split-class operands s (1 + q 2^-12) for the bf16x3 ones.  Every comparison of those is
torch.equal against a float64 reference -- a row dropped or doubled at a slice boundary, a column sum off by one row, a
missing cross-term MFMA in one tile are each a non-zero difference, where a maximum-relative error on Gaussian data
(test_train_gpu.py::test_gemms, the accuracy check at workload shapes) moves by 1 / K.  Operands sit in NaN-poisoned buffers
and C between sentinels, so strides, unaligned bases, column windows and ldc > N are checked for reads and writes that
leave their matrix.  The last tests bound the error on random floats per ELEMENT."""
import ctypes as C
import itertools

import pytest
import torch

from tests import gemm_reference as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (entry-point arithmetic, operand class): the split class is exact on the bf16x3 kernels only
ARITH = [("f32", "int"), ("bf16x3", "int"), ("bf16x3", "split")]
ARITH_IDS = [f"{p}-{c}" for p, c in ARITH]


def _hip():
    from multiply_amd import hip
    return hip


def _vp(ptr):
    return None if ptr is None else C.c_void_p(int(ptr))


def _same(got, want64):
    """bit-for-bit: the fp32 result, widened, IS the float64 reference (NaN anywhere fails)"""
    return torch.equal(got.double(), want64)


def _dev(x):
    return x.to(DEV)


# ====================================================================================================================== nt
def _gemm_nt(precision, A, lda, B, ldb, Cm, ldc, M, N, K, bias=None, bias_rows=0, accumulate=False, relu=False):
    hip = _hip()
    fn = hip.lib().mp_gemm_nt if precision == "f32" else hip.lib().mp_gemm_nt_bf16x3
    fn(_vp(A), lda, _vp(B), ldb, _vp(Cm), ldc, M, N, K, _vp(bias), bias_rows, int(accumulate), int(relu), hip.stream())


def _up4(k):
    return (k + 3) // 4 * 4


def _odd(k):
    return k + 1 if k % 2 == 0 else k + 2


# name -> (applies(K), lda(K), A's float offset, ldb(K), B's float offset, ldc - N)
NT_LAYOUTS = {
    "contiguous": (lambda K: True, lambda K: K, 0, lambda K: K, 0, 0),            # K % 32 == 0: the FAST path (M = 200: clamped rows)
    "ld+4": (lambda K: True, lambda K: _up4(K) + 4, 0, lambda K: _up4(K) + 4, 0, 5),  # 16 B aligned rows with a NaN margin
    "ld odd": (lambda K: True, _odd, 0, _odd, 0, 0),                             # every load through ld4's partial branch
    "feature read": (lambda K: K == 256, lambda K: 257, 1, lambda K: K, 0, 5),    # RenderTrain: off(Z8, 1), row stride 257
    "W window": (lambda K: K == 256, lambda K: K, 0, lambda K: 270, 14, 0),       # colour layer 0: off(W, c_feat), ldb = 270
    "ldc+5": (lambda K: True, lambda K: K, 0, lambda K: K, 0, 5),
}
NT_SHAPES = [(1, 1, 1), (5, 3, 7), (127, 129, 31), (128, 128, 32), (129, 127, 33), (257, 256, 64), (300, 3, 256), (200, 256, 256)]


@pytest.mark.parametrize("precision,cls", ARITH, ids=ARITH_IDS)
@pytest.mark.parametrize("layout", list(NT_LAYOUTS))
def test_nt_exact(precision, cls, layout):
    applies, lda_of, a_off, ldb_of, b_off, c_pad = NT_LAYOUTS[layout]
    terms = G.terms_of(cls)
    n_run = 0
    for si, (M, N, K) in enumerate(NT_SHAPES):
        if not applies(K):
            continue
        A = G.Embedded(_dev(G.operand(cls, M, K, 100 + si)), lda_of(K), a_off)
        B = G.Embedded(_dev(G.operand(cls, N, K, 200 + si)), ldb_of(K), b_off)
        assert (A.data_ptr() % 16 == 0) == (a_off % 4 == 0) and (B.data_ptr() % 16 == 0) == (b_off % 4 == 0)
        bias = G.GuardedVec(_dev(G.int_values((N,), 300 + si)))
        c0 = _dev(G.int_values((M, N), 400 + si))
        Cg = G.GuardedC(c0, N + c_pad)
        prod = G.product_nt(A.view, B.view, terms)
        for bias_rows, (accumulate, relu) in itertools.product((0, 1, 64, M), ((0, 0), (1, 0), (0, 1), (1, 1))):
            Cg.reset(c0)
            _gemm_nt(precision, A.data_ptr(), A.ld, B.data_ptr(), B.ld, Cg.data_ptr(), Cg.ldc, M, N, K,
                     bias.data_ptr() if bias_rows else None, bias_rows, accumulate, relu)
            want = G.epilogue_nt(prod, bias.buf[:N], bias_rows, c0, accumulate, relu)
            assert _same(Cg.check(), want), (M, N, K, bias_rows, accumulate, relu)
            n_run += 1
        bias.check()
    assert n_run >= 32


# ====================================================================================================================== tn
def _gemm_tn(precision, A, lda, B, ldb, Cm, ldc, M, N, K, colsum=None, colsum_rows=0):
    hip = _hip()
    fn = hip.lib().mp_gemm_tn if precision == "f32" else hip.lib().mp_gemm_tn_bf16x3
    fn(_vp(A), lda, _vp(B), ldb, _vp(Cm), ldc, M, N, K, _vp(colsum), colsum_rows, hip.stream())


def _tn_boundaries(M, N, K):
    """first and last row-slice boundary of a single tn launch.  Host formula (mp_gemm_tn*): tiles = ceil(M / 128) ceil(N / 128),
    slices = ceil(512 / tiles), rows = ceil(K / slices) rounded up to a multiple of 32, at least 128; slice z covers rows
    [z rows, min(K, (z + 1) rows))."""
    rows, slices = G.tn_rows_per_block(M, N, K)
    return [b for b in {rows, (slices - 1) * rows} if 0 < b < K]


# operand / output layouts of the tn cases: (lda - M | None = odd, ldb - N | "feat", ldc - N, C's column offset, colsum: float offset | None)
TN_VARIANTS = {
    "contiguous": (0, 0, 0, 0, 0),
    "ldc+5, colsum+1": (0, 0, 5, 0, 1),                # the grouped bias sum goes to off(db, 1)
    "C window": (0, 0, 14, 14, 0),                     # off(dW, c_feat) with ldc = in_dim > N
    "no colsum": (4, 4, 0, 0, None),                   # aligned rows with a NaN margin
    "odd strides": (None, "feat", 5, 0, 1),            # B = the production feature read: base + 1 float, odd row stride
}
TN_SHAPES = [(1, 32, 256), (3, 256, 500), (128, 128, 1), (128, 128, 127), (128, 128, 129), (256, 256, 4000), (257, 39, 3000),
             (130, 130, 33)]


def _tn_case(precision, cls, M, N, K, seed, variants=TN_VARIANTS):
    terms = G.terms_of(cls)
    a, b = _dev(G.operand(cls, K, M, seed)), _dev(G.operand(cls, K, N, seed + 1))
    c0, cs0 = _dev(G.int_values((M, N), seed + 2)), _dev(G.int_values((M,), seed + 3))
    prod = c0.double() + G.product_tn(a, b, terms)
    bounds = _tn_boundaries(M, N, K)
    all_rows = G.colsum_row_cases(K, bounds)
    for name, (da, db_, dc, col0, cs_off) in variants.items():
        A = G.Embedded(a, _odd(M) if da is None else M + da)
        B = G.Embedded(b, N + 1, 1) if db_ == "feat" else G.Embedded(b, N + db_)
        Cg = G.GuardedC(c0, N + dc, col0)
        # the full sweep of colsum_rows on the contiguous layout; the others at a slice boundary + 1 (or K - 1)
        sweep = all_rows if name == "contiguous" else [min(bounds) + 1 if bounds else K - 1]
        for rows in sweep:
            Cg.reset(c0)
            cs = None if cs_off is None else G.GuardedVec(cs0, cs_off)
            _gemm_tn(precision, A.data_ptr(), A.ld, B.data_ptr(), B.ld, Cg.data_ptr(), Cg.ldc, M, N, K,
                     None if cs is None else cs.data_ptr(), rows)
            assert _same(Cg.check(), prod), (M, N, K, name, rows)
            if cs is not None:
                assert _same(cs.check(), cs0.double() + a[:rows].double().sum(0)), (M, N, K, name, "colsum_rows", rows)


@pytest.mark.parametrize("precision,cls", ARITH, ids=ARITH_IDS)
@pytest.mark.parametrize("shape", TN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tn_exact(precision, cls, shape):
    M, N, K = shape          # (1, 32, 256) contiguous is _layer0_adjoint's M = 1, lda = 1
    _tn_case(precision, cls, M, N, K, 1000 + 10 * TN_SHAPES.index(shape))


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_tn_exact_many_slices(precision):
    """K = 100001 over a 256 x 256 output: 126 slices of 800 rows, the last one a single row (integer class: 64 K < 2^24)"""
    M, N, K = 256, 256, 100001
    rows, slices = G.tn_rows_per_block(M, N, K)
    assert (rows, slices) == (800, 126) and K - (slices - 1) * rows == 1
    _tn_case(precision, "int", M, N, K, 2000, {k: TN_VARIANTS[k] for k in ("contiguous", "ldc+5, colsum+1")})


# ================================================================================================================= grouped
class _Group:
    """one contraction of a grouped launch with its buffers and its float64 reference"""

    def __init__(self, cls, a, b, M, N, K, seed, lda=None, ldb=None, ldc_pad=0, col0=0, colsum_rows=None, cs_off=0, share=None,
                 a_ptr=None, b_ptr=None):
        self.M, self.N, self.K, self.a, self.b = M, N, K, a, b
        if a_ptr is None:                        # its own poisoned copies; else rows of a shared pair of buffers
            self.A, self.B = G.Embedded(a, lda or M), G.Embedded(b, ldb or N)
            a_ptr, b_ptr, lda, ldb = self.A.data_ptr(), self.B.data_ptr(), self.A.ld, self.B.ld
        self.a_ptr, self.b_ptr, self.lda, self.ldb = a_ptr, b_ptr, lda, ldb
        self.prod = G.product_tn(a, b, G.terms_of(cls))
        self.share = share
        if share is None:
            self.c0 = _dev(G.int_values((M, N), seed))
            self.Cg = G.GuardedC(self.c0, N + col0 + ldc_pad, col0)
            self.want = self.c0.double() + self.prod
        else:                                    # adds into another group's C
            self.Cg = share.Cg
            share.want = share.want + self.prod
        self.colsum_rows = colsum_rows
        self.cs = None
        if colsum_rows is not None:
            self.cs0 = _dev(G.int_values((M,), seed + 1))
            self.cs = G.GuardedVec(self.cs0, cs_off)

    def record(self):
        from multiply_amd import train as T
        return T.tn_group(_vp(self.a_ptr), self.lda, _vp(self.b_ptr), self.ldb, _vp(self.Cg.data_ptr()), self.Cg.ldc, self.M, self.N,
                          self.K, None if self.cs is None else _vp(self.cs.data_ptr()), self.colsum_rows or 0)

    def check(self, tag):
        if self.share is None:
            assert _same(self.Cg.check(), self.want), (tag, "C")
        if self.cs is not None:
            assert _same(self.cs.check(), self.cs0.double() + self.a[:self.colsum_rows].double().sum(0)), (tag, "colsum", self.colsum_rows)


def _launch_grouped(groups):
    from multiply_amd import train as T
    hip = _hip()
    recs = [g.record() for g in groups]
    arr = (T.MpTnGroup * len(recs))(*recs)
    return hip.lib().mp_gemm_tn_bf16x3_grouped(arr, len(recs), hip.stream())


CLASSES = ["int", "split"]


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("K", [1, 31, 32, 33, 255, 256, 257, 4000])
def test_grouped_wide_one_group(cls, K):
    """one 256 x 256 group: slices of max(256, ceil(K / 256) -> 32) rows (host formula of the wide form); colsum_rows over the
    ends, a stage +-1 and the first / last slice boundary +-1"""
    rows, per, _ = G.wide_rows_per_block([K])
    assert rows == 256 and per == [(K + 255) // 256]
    a, b = _dev(G.operand(cls, K, 256, 3000 + K)), _dev(G.operand(cls, K, 256, 3001 + K))
    bounds = [x for x in {rows, (per[0] - 1) * rows} if 0 < x < K]
    for i, cr in enumerate(G.colsum_row_cases(K, bounds) + [None]):
        g = _Group(cls, a, b, 256, 256, K, 3100 + i, ldc_pad=(0, 5)[i % 2], col0=(0, 14)[i % 3 == 2], colsum_rows=cr, cs_off=i % 2)
        _launch_grouped([g])
        g.check((K, cr))


@pytest.mark.parametrize("cls", CLASSES)
def test_grouped_wide_two_sweeps_share_c(cls):
    """K = (700, 1, 3000): the first two add into ONE C (a layer's value sweep and gradient sweep both go to dW_full); only the
    first carries a column sum"""
    Ks = (700, 1, 3000)
    ops = [(_dev(G.operand(cls, k, 256, 3200 + 2 * i)), _dev(G.operand(cls, k, 256, 3201 + 2 * i))) for i, k in enumerate(Ks)]
    for cr in (0, 255, 256, 257, 699, 700):          # slices are 256 rows here (asserted below)
        assert G.wide_rows_per_block(Ks)[0] == 256
        g0 = _Group(cls, *ops[0], 256, 256, Ks[0], 3300, ldc_pad=5, colsum_rows=cr, cs_off=1)
        g1 = _Group(cls, *ops[1], 256, 256, Ks[1], 3310, share=g0)
        g2 = _Group(cls, *ops[2], 256, 256, Ks[2], 3320, col0=14)
        _launch_grouped([g0, g1, g2])
        for i, g in enumerate((g0, g1, g2)):
            g.check((cr, i))


def _groups_of_buffers(cls, Ks, seed, bound):
    """len(Ks) 256 x 256 groups cut from ONE pair of operand buffers [sum K][256] (every row offset is 1 KiB aligned); each group
    has its own C and a column sum with its own row count (bound: the launch's slice length)"""
    tot = sum(Ks)
    a, b = _dev(G.operand(cls, tot, 256, seed)), _dev(G.operand(cls, tot, 256, seed + 1))
    A, B = G.Embedded(a, 256), G.Embedded(b, 256)
    groups, r0 = [], 0
    for i, k in enumerate(Ks):
        cr = (0, 1, k - 1, k, bound - 1, bound, bound + 1, 33)[i % 8]
        groups.append(_Group(cls, a[r0:r0 + k], b[r0:r0 + k], 256, 256, k, seed + 10 + 2 * i, lda=256, ldb=256, ldc_pad=(0, 5)[i % 2],
                             colsum_rows=min(cr, k), cs_off=i % 2, a_ptr=A.row_ptr(r0), b_ptr=B.row_ptr(r0)))
        r0 += k
    return groups, (A, B)


@pytest.mark.parametrize("cls", CLASSES)
def test_grouped_wide_24_groups(cls):
    """24 groups of ~2900 rows: 69 k rows in all, so the first slice length (288 rows: 11 slices per group = 264 > 256
    workgroups) does not fit one round and the host lengthens the slices"""
    Ks = [2900 + 4 * ((7 * i) % 5) - 8 for i in range(24)]
    assert len(Ks) == G.TN_MAX_GROUPS and sum(Ks) > 65536 and max(Ks) <= G.SPLIT_K_MAX
    rows, per, lengthened = G.wide_rows_per_block(Ks)
    assert lengthened >= 1 and sum(per) <= G.TNW_WGS, (rows, per, lengthened)      # the `while (z > MP_TNW_WGS)` loop is taken
    groups, keep = _groups_of_buffers(cls, Ks, 3400, rows)
    _launch_grouped(groups)
    for i, g in enumerate(groups):
        g.check(i)


@pytest.mark.parametrize("cls", CLASSES)
def test_grouped_25_groups_through_train(cls):
    """train.gemm_tn_grouped cuts 25 records into launches of 24 and 1: every group is computed"""
    from multiply_amd import train as T
    Ks = [40 + 13 * i for i in range(25)]
    assert G.wide_rows_per_block(Ks[:24])[0] == 256 and G.wide_rows_per_block(Ks[24:])[0] == 256
    groups, keep = _groups_of_buffers(cls, Ks, 3500, 256)
    T.gemm_tn_grouped([g.record() for g in groups])
    for i, g in enumerate(groups):
        g.check(i)


TILED_SHAPES = [(128, 128), (256, 128), (128, 256), (384, 128), (256, 256)]
TILED_K = (700, 300, 1500, 33, 257)


def _tiled_groups(cls, seed):
    groups = []
    for i, ((M, N), K) in enumerate(zip(TILED_SHAPES, TILED_K)):
        a, b = _dev(G.operand(cls, K, M, seed + 2 * i)), _dev(G.operand(cls, K, N, seed + 2 * i + 1))
        cr = {0: 257, 2: 1279, 3: K}.get(i)           # column sums on some groups only; 256 = the slice length (asserted)
        groups.append(_Group(cls, a, b, M, N, K, seed + 20 + 2 * i, lda=M + 4 * (i % 2), ldb=N + 4 * (i % 3 == 0), ldc_pad=5,
                             col0=(0, 14)[i % 2], colsum_rows=cr, cs_off=int(i == 2)))
    return groups


@pytest.mark.parametrize("cls", CLASSES)
def test_grouped_tiled(cls):
    """groups that are not all 256 x 256 take k_gemm_tn_b3g (128 x 128 tiles; workgroup L -> slice (L & 7) + 8 (L / (8 tiles)),
    tile (L >> 3) % tiles).  mt x nt = 3 x 2 are maxima most groups do not fill; 14 slices: a padded grid of 16"""
    assert any(s != (256, 256) for s in TILED_SHAPES)
    rows, per, mt, nt = G.tiled_rows_per_block(TILED_SHAPES, TILED_K)
    z = sum(per)
    assert rows == 256 and (mt, nt) == (3, 2) and z == 14 and z > 8 and z % 8 != 0
    assert sum(m // 128 * (n // 128) < mt * nt for m, n in TILED_SHAPES) == len(TILED_SHAPES)   # no group fills the tile grid
    groups = _tiled_groups(cls, 3600)
    _launch_grouped(groups)
    for i, g in enumerate(groups):
        g.check(i)


# ========================================================================================================= status contract
def _status_group(**kw):
    K = kw.pop("K", 64)
    M = kw.pop("M", 256)
    a, b = _dev(G.operand("int", max(K, 1), M, 3700)), _dev(G.operand("int", max(K, 1), 256, 3701))
    return _Group("int", a[:K], b[:K], M, 256, K, 3702, **kw)


def test_grouped_status_contract():
    """what include/multiply_hip.h documents for mp_gemm_tn_bf16x3_grouped: 0 groups = no-op; more than MP_TN_MAX_GROUPS = -1;
    a group with a shape or an operand layout the kernels do not take -- M (N) no multiple of 128, lda (ldb) no multiple of 4,
    A (B) not 16-byte aligned, or an EMPTY contraction (K <= 0) -- = -2 for the whole call.  No launch happens in any of them."""
    hip = _hip()
    assert hip.lib().mp_gemm_tn_bf16x3_grouped(None, 0, hip.stream()) == 0
    good = _status_group()

    def refused(groups, code):
        with pytest.raises(RuntimeError, match=rf"mp_gemm_tn_bf16x3_grouped failed with code {code}$"):
            _launch_grouped(groups)
        torch.cuda.synchronize()
        assert torch.equal(good.Cg.check(), good.c0)          # nothing was launched: the valid group's C is untouched

    refused([good] * 25, -1)
    refused([good, _status_group(M=192)], -2)
    refused([good, _status_group(lda=258)], -2)
    odd = _status_group()
    odd.a_ptr += 4                                           # A one float past a 16-byte boundary (the margin row keeps it in bounds)
    refused([good, odd], -2)
    refused([good, _status_group(K=0)], -2)                  # the trainer never builds one: a person keeps >= 1 ray and 512 eikonal points
    _launch_grouped([good])                                  # and the valid group on its own is computed
    good.check("good")


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_tn_empty_contraction_is_a_noop(precision):
    """the single-launch entry points return 0 without a launch for K <= 0 (and M or N <= 0)"""
    g = _status_group()
    for M, N, K in ((256, 256, 0), (0, 256, 64), (256, 0, 64)):
        _gemm_tn(precision, g.a_ptr, 256, g.b_ptr, 256, g.Cg.data_ptr(), g.Cg.ldc, M, N, K, None, 0)
    torch.cuda.synchronize()
    assert torch.equal(g.Cg.check(), g.c0)


# ========================================================================================== random floats, per element
def _float_pairs(rows_a, cols_a, rows_b, cols_b, seed):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(rows_a, cols_a, generator=g), torch.randn(rows_b, cols_b, generator=g)
    return {"gaussian": (_dev(a), _dev(b)), "1e-9 x 1e+6": (_dev(a * 1e-9), _dev(b * 1e6))}


def _assert_float_bound(tag, got, want64, abs_prod, K, split):
    bound = G.float_bound(abs_prod, K, split)
    r = G.worst_ratio(got, want64, bound)
    print(f"[gemm float bound] {tag}: worst |err| / bound = {r:.2e}")
    assert bool((got.double() - want64).abs().le(bound).all()), (tag, r)


# Per element: |got - want64| <= (4 x 2^-18 [bf16x3] + (K + 8) 2^-23) (|A|^T |B|)  (G.float_bound: split residuals and the dropped
# lo.lo term; one ulp per accumulated term; a few atomic adds).  Derived, not tuned.
@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_nt_random_floats(precision):
    # measured worst |err| / bound (MI355X): f32 9.3e-3 (gaussian), 8.5e-3 (1e-9 x 1e+6); bf16x3 4.8e-2, 4.4e-2
    M, N, K = 300, 256, 256
    for name, (a, b) in _float_pairs(M, K, N, K, 3800).items():
        Cm = torch.full((M, N), float("nan"), device=DEV)
        _gemm_nt(precision, a.data_ptr(), K, b.data_ptr(), K, Cm.data_ptr(), N, M, N, K)
        _assert_float_bound(f"nt[{precision}] {name}", Cm, a.double() @ b.double().T, a.double().abs() @ b.double().abs().T, K,
                            precision == "bf16x3")


@pytest.mark.parametrize("entry", ["f32", "bf16x3", "grouped"])
def test_tn_random_floats(entry):
    # measured worst |err| / bound (MI355X): f32 1e-4 (gaussian), 9e-5 (1e-9 x 1e+6); bf16x3 and grouped 1.6e-3, 1.4e-3
    M, N, K = 256, 256, 3000
    for name, (a, b) in _float_pairs(K, M, K, N, 3900).items():
        Cm = torch.zeros(M, N, device=DEV)
        if entry == "grouped":
            from multiply_amd import train as T
            T.gemm_tn_grouped([T.tn_group(_vp(a.data_ptr()), M, _vp(b.data_ptr()), N, _vp(Cm.data_ptr()), N, M, N, K)])
        else:
            _gemm_tn(entry, a.data_ptr(), M, b.data_ptr(), N, Cm.data_ptr(), N, M, N, K)
        _assert_float_bound(f"tn[{entry}] {name}", Cm, a.double().T @ b.double(), a.double().abs().T @ b.double().abs(), K,
                            entry != "f32")
