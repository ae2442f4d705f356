"""Exact-input references of the training GEMMs (csrc/gemm.hip).  torch and numpy only: no GPU, no project imports.

A GEMM has no discontinuity, so with suitable operands its fp32 result is EXACT -- bit-identical to a float64 / int64
reference whatever the summation order, the number of row slices or the order of the atomics -- and any indexing mistake
(a row dropped or counted twice at a slice boundary, a tile taken from the wrong place, a missing MFMA) is a non-zero
difference.  Two classes of operands:

  integer  entries are integers in [-8, 8].  bfloat16 holds them exactly (hi = x, lo = 0), every product and every partial
           sum is an integer of magnitude <= 64 K + |C0| + |bias| < 2^24 for K <= 262143: exact in both GEMM arithmetics.
  split    entries are s (1 + q 2^-12), s = +-1, q an integer in [-7, 7] (q = +-8 would be a rounding tie).  Then
           hi = bf16(x) = s and lo = bf16(x - hi) = s q 2^-12 exactly; each of the three MFMA terms hi.hi, hi.lo, lo.hi is a
           multiple of 2^-12 and every partial sum is one of magnitude < 2^12 for K <= 4000 (with |C0| <= 8): exact in fp32.
           The split-bf16 kernels must return exactly hi^T hi + hi^T lo + lo^T hi; the full product differs from that by
           the dropped lo.lo term (multiples of 2^-24: ~14 fp32 ulps at K = 4000), so a missing or doubled cross term, a
           cross term from the wrong tile, and an included lo.lo all show.  (The exact-fp32 kernels would have to hold
           the 2^-24 multiples too, which fp32 cannot: this class is for the bf16x3 entry points only.)

Layout helpers put the operands into larger buffers whose every other element is NaN (operands) or a sentinel bit pattern
(C), all inside the test's own allocation: a kernel that reads one element too many turns its output into NaN, one that
writes outside its window changes a sentinel -- neither can fault.
"""
import numpy as np
import torch

INT_MAX_ABS = 8                 # integer class: entries in [-8, 8]
SPLIT_Q_MAX = 7                 # split class: q in [-7, 7]
SPLIT_LO_SCALE = 2.0 ** -12
INT_K_MAX = 262143              # 64 K < 2^24
SPLIT_K_MAX = 4000              # K (1 + 14 / 4096) + 8 < 2^12
SENTINEL = 0x7FA5C3D2           # a NaN bit pattern: an atomic add to it, or a store of anything else, changes the bits

# the tile and launch constants of csrc/gemm.hip that the slice arithmetic below repeats
BM = BN = 128
BK = 32
TN_WGS = 512                    # mp_gemm_tn / mp_gemm_tn_bf16x3: workgroups a contraction is split into
TNW_WGS = 256                   # wide grouped launch: one workgroup per CU
TNG_WGS = 1024                  # tiled grouped launch
TN_MAX_GROUPS = 24


# ---------------------------------------------------------------------------------------------------------------- operands
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def int_operand(rows, cols, seed):
    """-> (x fp32 [rows][cols], its integers int64)"""
    q = torch.randint(-INT_MAX_ABS, INT_MAX_ABS + 1, (rows, cols), generator=_gen(seed), dtype=torch.int64)
    return q.to(torch.float32), q


def split_operand(rows, cols, seed):
    """-> (x fp32 = s (1 + q 2^-12), s int64 in {-1, 1}, q int64 in [-7, 7])"""
    g = _gen(seed)
    s = 2 * torch.randint(0, 2, (rows, cols), generator=g, dtype=torch.int64) - 1
    q = torch.randint(-SPLIT_Q_MAX, SPLIT_Q_MAX + 1, (rows, cols), generator=g, dtype=torch.int64)
    x = s.double() * (1.0 + q.double() * SPLIT_LO_SCALE)          # 13 significant bits: exact in fp32
    return x.to(torch.float32), s, q


def operand(cls, rows, cols, seed):
    """fp32 operand of class 'int' | 'split'"""
    return (int_operand if cls == "int" else split_operand)(rows, cols, seed)[0]


def int_values(shape, seed, max_abs=INT_MAX_ABS):
    """integer-valued fp32 tensor (bias, initial C, initial column sums)"""
    return torch.randint(-max_abs, max_abs + 1, tuple(shape), generator=_gen(seed), dtype=torch.int64).to(torch.float32)


def split_bf16(x):
    """the kernels' split: hi = bf16(x), lo = bf16(x - hi), both returned as fp32"""
    hi = x.to(torch.bfloat16).to(torch.float32)
    lo = (x - hi).to(torch.bfloat16).to(torch.float32)
    return hi, lo


# -------------------------------------------------------------------------------------------------------------- references
def product_nt(A, B, terms="full"):
    """A [M][K] . B [N][K]^T in float64.  terms 'full': the product itself (exact for the integer class; the float64 reference
    of random data);  'three': hi.hi + hi.lo + lo.hi of the bf16 split (what the bf16x3 kernels compute, exact for the split
    class)."""
    if terms == "full":
        return A.double() @ B.double().T
    assert terms == "three"
    (ah, al), (bh, bl) = split_bf16(A), split_bf16(B)
    ah, al, bh, bl = ah.double(), al.double(), bh.double(), bl.double()
    return ah @ bh.T + ah @ bl.T + al @ bh.T


def product_tn(A, B, terms="full"):
    """A [K][M]^T . B [K][N] in float64"""
    return product_nt(A.T, B.T, terms)


def terms_of(cls):
    return "three" if cls == "split" else "full"


def epilogue_nt(P, bias=None, bias_rows=0, c0=None, accumulate=False, relu=False):
    """mp_gemm_nt's epilogue on a float64 product P [M][N]: bias on rows < bias_rows, then + C0, then ReLU"""
    out = P.clone()
    if bias is not None and bias_rows > 0:
        out[:min(bias_rows, out.shape[0])] += bias.double()
    if accumulate:
        out += c0.double()
    if relu:
        out = out.clamp_min(0.0)
    return out


def ref_nt(A, B, terms="full", bias=None, bias_rows=0, c0=None, accumulate=False, relu=False):
    return epilogue_nt(product_nt(A, B, terms), bias, bias_rows, c0, accumulate, relu)


def ref_tn(A, B, c0, terms="full", colsum0=None, colsum_rows=0):
    """-> (C0 + A^T B, colsum0 + column sums of A's first colsum_rows rows | None), float64"""
    Cw = c0.double() + product_tn(A, B, terms)
    cs = None if colsum0 is None else colsum0.double() + A[:max(colsum_rows, 0)].double().sum(0)
    return Cw, cs


def ref_nt_int64(Aq, Bq, bias=None, bias_rows=0, c0=None, accumulate=False, relu=False):
    """the integer class in int64 (host tensors)"""
    out = Aq @ Bq.T
    if bias is not None and bias_rows > 0:
        out[:min(bias_rows, out.shape[0])] += bias
    if accumulate:
        out = out + c0
    return out.clamp_min(0) if relu else out


# ------------------------------------------------------------------------------------------------------------------ layouts
class Embedded:
    """a logical [rows][width] operand inside a larger NaN-filled buffer: element (r, c) at float `offset + r ld + c` past a
    16-byte aligned origin, so that `offset` alone decides the pointer's alignment.  NaN everywhere else: before the first
    element, in the columns [width, ld) of every row, and in `margin_rows` rows past the last."""

    def __init__(self, x, ld, offset=0, margin_rows=1, device=None):
        rows, width = x.shape
        assert ld >= width or rows == 1
        dev = x.device if device is None else device
        lead = 64                                              # floats of NaN in front (256 bytes: alignment unchanged)
        n = lead + offset + (rows + margin_rows) * max(ld, width) + 64
        self.buf = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
        self.ld, self.offset, self.rows, self.width = ld, offset, rows, width
        self.first = lead + offset                            # index of element (0, 0) in buf
        self.view = torch.as_strided(self.buf, (rows, width), (ld, 1), self.first)
        self.view.copy_(x)

    def data_ptr(self):
        assert self.buf.data_ptr() % 16 == 0
        return self.buf.data_ptr() + 4 * self.first

    def row_ptr(self, r):
        return self.data_ptr() + 4 * r * self.ld


class GuardedC:
    """C [M][N] as a window at column `col0` of rows of width ldc >= col0 + N, with one guard row before and one after; every
    float outside the window holds SENTINEL.  check() asserts that each of them is bit-unchanged and returns the window."""

    def __init__(self, c0, ldc, col0=0, device=None):
        M, N = c0.shape
        assert ldc >= col0 + N
        dev = c0.device if device is None else device
        self.M, self.N, self.ldc, self.col0 = M, N, ldc, col0
        self.bits = torch.full(((M + 2) * ldc,), SENTINEL, dtype=torch.int32, device=dev)
        self.buf = self.bits.view(torch.float32)
        self.window = self.buf.view(M + 2, ldc)[1:M + 1, col0:col0 + N]
        self.window.copy_(c0)
        self.outside = torch.ones(M + 2, ldc, dtype=torch.bool, device=dev)
        self.outside[1:M + 1, col0:col0 + N] = False

    def data_ptr(self):
        return self.buf.data_ptr() + 4 * (self.ldc + self.col0)

    def reset(self, c0):
        self.bits.fill_(SENTINEL)
        self.window.copy_(c0)

    def sentinels_intact(self):
        return bool((self.bits.view(self.M + 2, self.ldc)[self.outside] == SENTINEL).all())

    def check(self):
        assert self.sentinels_intact(), "a write landed outside C's window"
        return self.window.clone()


class GuardedVec:
    """a vector (column sums, bias) at float `offset` of a sentinel-filled buffer"""

    def __init__(self, v0, offset=0, device=None):
        n = v0.numel()
        dev = v0.device if device is None else device
        self.n, self.offset = n, offset
        self.bits = torch.full((offset + n + 64,), SENTINEL, dtype=torch.int32, device=dev)
        self.buf = self.bits.view(torch.float32)
        self.buf[offset:offset + n].copy_(v0)

    def data_ptr(self):
        return self.buf.data_ptr() + 4 * self.offset

    def check(self):
        b = self.bits
        assert bool((b[:self.offset] == SENTINEL).all()) and bool((b[self.offset + self.n:] == SENTINEL).all()), \
            "a write landed outside the vector"
        return self.buf[self.offset:self.offset + self.n].clone()


# ------------------------------------------------------------------------------------- the host side's slice arithmetic
def _ceil(a, b):
    return (a + b - 1) // b


def tn_rows_per_block(M, N, K, wgs=TN_WGS):
    """rows per slice and slice count of mp_gemm_tn / mp_gemm_tn_bf16x3: enough slices that tiles x slices >= wgs, rounded up
    to whole 32-row stages, at least 4 stages each"""
    tiles = _ceil(M, BM) * _ceil(N, BN)
    slices = _ceil(wgs, tiles)
    rows = _ceil(_ceil(K, slices), BK) * BK
    rows = max(rows, 4 * BK)
    return rows, _ceil(K, rows)


def wide_rows_per_block(Ks, wgs=TNW_WGS):
    """mp_gemm_tn_bf16x3_grouped, wide form (every group 256 x 256) -> (rows per slice, slices per group, how often the host
    had to lengthen the slices before all groups' rounded-up slice counts fit one round of workgroups)"""
    work = sum(4 * k for k in Ks)
    rows = _ceil(_ceil(work // 4, wgs), BK) * BK
    rows = max(rows, 8 * BK)
    lengthened = 0
    while sum(_ceil(k, rows) for k in Ks) > wgs:
        rows += BK
        lengthened += 1
    return rows, [_ceil(k, rows) for k in Ks], lengthened


def tiled_rows_per_block(shapes, Ks, wgs=TNG_WGS):
    """the same for the tiled form (128 x 128 tiles); shapes = [(M, N)] -> (rows per slice, slices per group, mt, nt)"""
    tiles = [(m // BM) * (n // BN) for m, n in shapes]
    work = sum(t * k for t, k in zip(tiles, Ks))
    rows = _ceil(_ceil(work, wgs), BK) * BK
    rows = max(rows, 8 * BK)
    while sum(t * _ceil(k, rows) for t, k in zip(tiles, Ks)) > wgs:
        rows += BK
    return rows, [_ceil(k, rows) for k in Ks], max(m // BM for m, _ in shapes), max(n // BN for _, n in shapes)


def colsum_row_cases(K, boundaries=()):
    """colsum_rows values of a contraction over K rows: the ends, one MFMA stage +-1, and every given slice boundary +-1"""
    c = {0, 1, 31, 32, 33, K - 1, K}
    for b in boundaries:
        c |= {b - 1, b, b + 1}
    return sorted(x for x in c if 0 <= x <= K)


# ------------------------------------------------------------------------------------------------ random data, per element
def float_bound(A_abs_B_abs, K, split):
    """per-element error bound of a product against float64, as a multiple of (|A|^T |B|)[m][n]:
    split-bf16: hi keeps 8 significant bits and lo the next 8, so x - hi - lo is ~2^-18 |x| per operand (2^-17 at the very
    worst), and the dropped lo.lo term is of that size again: 4 x 2^-18 for the two residuals, the dropped term and their
    cross effects;  fp32 accumulation of K terms: one ulp (2^-23: the matrix instruction may truncate) per term, and 8 more
    for the few atomic adds / the epilogue.  Nothing here is fitted to what the kernels return."""
    return ((4.0 * 2.0 ** -18 if split else 0.0) + (K + 8) * 2.0 ** -23) * A_abs_B_abs


def worst_ratio(got, want64, bound):
    """max over the elements of |got - want| / bound (a zero bound with a zero error counts as 0)"""
    err = (got.double() - want64).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    return float(r.max())
