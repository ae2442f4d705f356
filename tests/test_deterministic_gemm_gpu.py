"""The deterministic forms of the weight-gradient contractions (csrc/gemm.hip: mp_gemm_tn_det, mp_gemm_tn_bf16x3_det,
mp_gemm_tn_bf16x3_grouped_det -- the tiled 128 x 128 and the wide 256 x 256 kernel): every row slice stores its partial tile into a
caller-provided workspace, a finishing kernel adds the slices in ascending order.

(a) exact operands (tests/gemm_reference.py): C and colsum equal the float64 reference bit for bit, on a C pre-filled with exact
    non-zero values;  (b) random fp32 operands: two launches give the same bits, the error against float64 is within the bound
    tests/test_gemm_gpu.py holds the atomic entry points to (gemm_reference.float_bound), and the words behind the workspace and
    around C are untouched."""
import ctypes as C

import pytest
import torch

from tests import gemm_reference as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
ARITH = [("f32", "int"), ("bf16x3", "int"), ("bf16x3", "split")]
ARITH_IDS = [f"{p}-{c}" for p, c in ARITH]


def _vp(ptr):
    return None if ptr is None else C.c_void_p(int(ptr))


class _Workspace:
    """exactly `n_bytes` of workspace with 64 sentinel words behind it"""

    def __init__(self, n_bytes):
        assert n_bytes % 4 == 0
        self.n = n_bytes // 4
        self.bits = torch.full((self.n + 64,), G.SENTINEL, dtype=torch.int32, device=DEV)
        self.n_bytes = n_bytes

    def ptr(self):
        assert self.bits.data_ptr() % 16 == 0
        return _vp(self.bits.data_ptr())

    def intact(self):
        return bool((self.bits[self.n:] == G.SENTINEL).all())


def _single_bytes(M, N, K, b3):
    from multiply_amd import hip
    need = C.c_longlong()
    hip.lib().mp_gemm_tn_ws_bytes(M, N, K, int(b3), C.byref(need))
    return int(need.value)


class _Case:
    """one contraction: operands a [K][M], b [K][N] in NaN-padded buffers of row strides lda / ldb, C in a sentinel-guarded window,
    optionally a guarded column-sum vector"""

    def __init__(self, a, b, c0, lda, ldb, ldc_pad, col0, colsum_rows, cs0, offset=0):
        self.a, self.b, self.c0, self.cs0, self.colsum_rows = a, b, c0, cs0, colsum_rows
        K, M = a.shape
        N = b.shape[1]
        self.M, self.N, self.K, self.lda, self.ldb = M, N, K, lda, ldb
        self.A, self.B = G.Embedded(a, lda, offset=offset), G.Embedded(b, ldb, offset=offset)
        self.Cg = G.GuardedC(c0, col0 + N + ldc_pad, col0)
        self.cs = None if colsum_rows is None else G.GuardedVec(cs0, offset=1)

    def reset(self):
        self.Cg.reset(self.c0)
        if self.cs is not None:
            self.cs.buf[self.cs.offset:self.cs.offset + self.cs.n].copy_(self.cs0)

    def args(self):
        return (_vp(self.A.data_ptr()), self.lda, _vp(self.B.data_ptr()), self.ldb, _vp(self.Cg.data_ptr()), self.Cg.ldc, self.M, self.N,
                self.K, None if self.cs is None else _vp(self.cs.data_ptr()), self.colsum_rows or 0)

    def record(self):
        from multiply_amd import train as T
        a = self.args()
        return T.tn_group(*a[:9], a[9], a[10])

    def launch_single(self, precision):
        from multiply_amd import hip
        ws = _Workspace(_single_bytes(self.M, self.N, self.K, precision != "f32"))
        fn = hip.lib().mp_gemm_tn_det if precision == "f32" else hip.lib().mp_gemm_tn_bf16x3_det
        fn(*self.args(), ws.ptr(), ws.n_bytes, hip.stream())
        torch.cuda.synchronize()
        assert ws.intact(), "a write landed behind the workspace"

    def results(self):
        return self.Cg.check(), None if self.cs is None else self.cs.check()


def _launch_grouped(cases):
    from multiply_amd import hip, train as T
    recs = [c.record() for c in cases]
    arr = (T.MpTnGroup * len(recs))(*recs)
    need = C.c_longlong()
    hip.lib().mp_gemm_tn_grouped_ws_bytes(arr, len(recs), C.byref(need))
    ws = _Workspace(int(need.value))
    hip.lib().mp_gemm_tn_bf16x3_grouped_det(arr, len(recs), ws.ptr(), ws.n_bytes, hip.stream())
    torch.cuda.synchronize()
    assert ws.intact(), "a write landed behind the workspace"


# the issue's shapes: (M, N, K, lda - M, ldb - N, ldc padding, column of C's window, colsum_rows, operand offset in floats)
SINGLE = {"three-slices-last-ragged": (128, 128, 296, 0, 0, 0, 0, 296, 0),
          "unaligned": (100, 36, 296, 1, 3, 5, 14, 200, 1)}
WIDE_K = (600, 256, 40)
TILED = ((128, 256, 300), (128, 256, 257))


def _exact_case(cls, M, N, K, dlda, dldb, ldc_pad, col0, colsum_rows, offset, seed):
    a, b = G.operand(cls, K, M, seed).to(DEV), G.operand(cls, K, N, seed + 1).to(DEV)
    c0 = G.int_values((M, N), seed + 2).to(DEV) + 1.0          # integers in [-7, 9]: exact, and no element is left at zero by chance alone
    cs0 = G.int_values((M,), seed + 3).to(DEV)
    return _Case(a, b, c0, M + dlda, N + dldb, ldc_pad, col0, colsum_rows, cs0, offset)


def _check_exact(case, cls, tag):
    Cw, cs = case.results()
    want, want_cs = G.ref_tn(case.a.cpu(), case.b.cpu(), case.c0.cpu(), G.terms_of(cls), case.cs0.cpu(), case.colsum_rows or 0)
    assert torch.equal(Cw.double().cpu(), want), (tag, "C")
    if cs is not None:
        assert torch.equal(cs.double().cpu(), want_cs), (tag, "colsum")


@pytest.mark.parametrize("shape", list(SINGLE))
@pytest.mark.parametrize("precision,cls", ARITH, ids=ARITH_IDS)
def test_single_launch_exact(precision, cls, shape):
    M, N, K = SINGLE[shape][:3]
    assert G.tn_rows_per_block(M, N, K) == (128, 3)            # three slices of 128 rows, the last one 40 rows
    case = _exact_case(cls, *SINGLE[shape], seed=7100)
    case.launch_single(precision)
    _check_exact(case, cls, (precision, cls, shape))


@pytest.mark.parametrize("cls", ["int", "split"])
def test_grouped_wide_exact(cls):
    """three 256 x 256 groups of K = 600, 256, 40: 256-row slices, 3 + 1 + 1 of them"""
    assert G.wide_rows_per_block(WIDE_K)[:2] == (256, [3, 1, 1])
    cases = [_exact_case(cls, 256, 256, K, 0, 0, (0, 5, 0)[i], (0, 0, 14)[i], (K, None, 33)[i], 0, 7200 + 10 * i) for i, K in enumerate(WIDE_K)]
    _launch_grouped(cases)
    for i, c in enumerate(cases):
        _check_exact(c, cls, ("wide", cls, i))


@pytest.mark.parametrize("cls", ["int", "split"])
def test_grouped_wide_two_groups_share_c(cls):
    """a layer's value sweep and gradient sweep add into the same dW: the finishing pass chains them, in the order of the groups"""
    from multiply_amd import train as T
    c1 = _exact_case(cls, 256, 256, 600, 0, 0, 5, 0, 600, 0, 7300)
    c2 = _exact_case(cls, 256, 256, 40, 0, 0, 5, 0, None, 0, 7310)
    a1 = c1.args()
    rec2 = T.tn_group(*c2.args()[:4], a1[4], a1[5], 256, 256, 40)
    from multiply_amd import hip
    arr = (T.MpTnGroup * 2)(c1.record(), rec2)
    need = C.c_longlong()
    hip.lib().mp_gemm_tn_grouped_ws_bytes(arr, 2, C.byref(need))
    ws = _Workspace(int(need.value))
    hip.lib().mp_gemm_tn_bf16x3_grouped_det(arr, 2, ws.ptr(), ws.n_bytes, hip.stream())
    torch.cuda.synchronize()
    assert ws.intact()
    t = G.terms_of(cls)
    want = c1.c0.cpu().double() + G.product_tn(c1.a.cpu(), c1.b.cpu(), t) + G.product_tn(c2.a.cpu(), c2.b.cpu(), t)
    assert torch.equal(c1.Cg.check().double().cpu(), want)
    assert torch.equal(c2.Cg.check(), c2.c0)                   # the second record's own C was never named: untouched


@pytest.mark.parametrize("cls", ["int", "split"])
def test_grouped_tiled_exact(cls):
    """two groups of M = 128, N = 256: not all 256 x 256, hence the 128 x 128-tile kernel"""
    rows, per, mt, nt = G.tiled_rows_per_block([(m, n) for m, n, _ in TILED], [k for _, _, k in TILED])
    assert (rows, mt, nt) == (256, 1, 2) and per == [2, 2]
    cases = [_exact_case(cls, M, N, K, 4 * i, 0, 5, (0, 14)[i], (K - 1, 257)[i], 0, 7400 + 10 * i) for i, (M, N, K) in enumerate(TILED)]
    _launch_grouped(cases)
    for i, c in enumerate(cases):
        _check_exact(c, cls, ("tiled", cls, i))


# ------------------------------------------------------------------------------------------------------------- random operands
def _float_case(M, N, K, dlda, dldb, ldc_pad, col0, colsum_rows, offset, seed):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(K, M, generator=g).to(DEV), torch.randn(K, N, generator=g).to(DEV)
    c0, cs0 = torch.zeros(M, N, device=DEV), torch.zeros(M, device=DEV)      # as tests/test_gemm_gpu.py applies the bound: onto zeros
    return _Case(a, b, c0, M + dlda, N + dldb, ldc_pad, col0, colsum_rows, cs0, offset)


def _check_float(case, split, tag):
    """the atomic entry points' bound (tests/test_gemm_gpu.py: gemm_reference.float_bound of |A|^T |B|) on C - C0; the column sums,
    exact-fp32 sums of colsum_rows terms in either arithmetic, against the same formula without the split's share"""
    Cw, cs = case.results()
    a, b = case.a.double().cpu(), case.b.double().cpu()
    want = case.c0.double().cpu() + a.T @ b
    bound = G.float_bound(a.abs().T @ b.abs(), case.K, split)
    r = G.worst_ratio(Cw.cpu(), want, bound)
    print(f"[deterministic gemm] {tag}: worst |err| / bound = {r:.2e}")
    assert bool((Cw.double().cpu() - want).abs().le(bound).all()), (tag, r)
    if cs is not None:
        rows = case.colsum_rows
        want_cs = case.cs0.double().cpu() + a[:rows].sum(0)
        bound_cs = G.float_bound(a[:rows].abs().sum(0), rows, False)
        assert bool((cs.double().cpu() - want_cs).abs().le(bound_cs).all()), (tag, "colsum")


@pytest.mark.parametrize("shape", list(SINGLE))
@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_single_launch_random_twice(precision, shape):
    case = _float_case(*SINGLE[shape], seed=7500)
    case.launch_single(precision)
    first = case.results()
    _check_float(case, precision != "f32", (precision, shape))
    case.reset()
    case.launch_single(precision)                              # (another workspace allocation: the address must not matter)
    second = case.results()
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


@pytest.mark.parametrize("form", ["wide", "tiled"])
def test_grouped_random_twice(form):
    if form == "wide":
        cases = [_float_case(256, 256, K, 0, 0, (0, 5, 0)[i], (0, 0, 14)[i], (K, None, 33)[i], 0, 7600 + 10 * i) for i, K in enumerate(WIDE_K)]
    else:
        cases = [_float_case(M, N, K, 4 * i, 0, 5, (0, 14)[i], (K - 1, 257)[i], 0, 7700 + 10 * i) for i, (M, N, K) in enumerate(TILED)]
    _launch_grouped(cases)
    first = [c.results() for c in cases]
    for i, c in enumerate(cases):
        _check_float(c, True, (form, i))
        c.reset()
    _launch_grouped(cases)
    for (c1, s1), c in zip(first, cases):
        c2, s2 = c.results()
        assert torch.equal(c1, c2) and (s1 is None or torch.equal(s1, s2))


def test_workspace_status_contract():
    """-3 and no launch: a NULL, a misaligned or a too small workspace; the size queries answer 0 for an empty contraction"""
    from multiply_amd import hip
    case = _exact_case("int", 128, 128, 296, 0, 0, 0, 0, 296, 0, 7800)
    need = _single_bytes(128, 128, 296, True)
    assert need == 4 * 3 * (128 * 128 + 128) and _single_bytes(128, 128, 0, True) == 0
    ws = _Workspace(need)
    for ptr, nbytes in ((None, need), (_vp(ws.bits.data_ptr() + 4), need), (ws.ptr(), need - 4)):
        with pytest.raises(RuntimeError, match=r"mp_gemm_tn_bf16x3_det failed with code -3$"):
            hip.lib().mp_gemm_tn_bf16x3_det(*case.args(), ptr, nbytes, hip.stream())
    torch.cuda.synchronize()
    assert torch.equal(case.Cg.check(), case.c0)
