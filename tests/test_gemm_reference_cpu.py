"""The premises of the exact-input GEMM tests (tests/gemm_reference.py, tests/test_gemm_gpu.py), checked on the host:
both operand classes are exact under the bf16 split and under fp32 accumulation in any order, the dropped lo.lo term of the
split class is visible, and the reference agrees with a plain triple loop."""
import itertools

import numpy as np
import pytest
import torch

from tests import gemm_reference as G


def _accumulate_fp32(terms, seed):
    """sequential fp32 sum of `terms` (fp32 numpy vector) in a random order"""
    order = np.random.default_rng(seed).permutation(terms.shape[0])
    acc = np.float32(0.0)
    for chunk in np.array_split(terms[order], 64):          # np.cumsum of a 1-D array is a sequential running sum
        acc = np.cumsum(np.concatenate([[acc], chunk]).astype(np.float32), dtype=np.float32)[-1]
    return acc


def test_split_class_premises():
    K = G.SPLIT_K_MAX
    A, sa, qa = G.split_operand(K, 6, 1)
    B, sb, qb = G.split_operand(K, 5, 2)
    for x, s, q in ((A, sa, qa), (B, sb, qb)):
        hi, lo = G.split_bf16(x)
        assert torch.equal(hi, s.float())                                   # hi = s exactly
        assert torch.equal(lo, (s * q).float() * G.SPLIT_LO_SCALE)          # lo = s q 2^-12 exactly
        assert torch.equal(hi + lo, x)
        assert torch.equal(lo.to(torch.bfloat16).float(), lo) and torch.equal(hi.to(torch.bfloat16).float(), hi)
    want = G.product_tn(A, B, "three")
    # the same in integers: 2^12 (hi hi + hi lo + lo hi) = s s' (4096 + q + q')
    units = torch.einsum("km,kn->mn", sa, sb * 4096) + torch.einsum("km,kn->mn", sa * qa, sb) + torch.einsum("km,kn->mn", sa, sb * qb)
    assert torch.equal(want, units.double() / 4096.0)
    assert float(want.abs().max()) + G.INT_MAX_ABS < 4096.0                 # every partial sum below 2^12 at resolution 2^-12
    # fp32 accumulation of the 3 K MFMA terms of single elements, two random orders: bit-identical to float64
    (ah, al), (bh, bl) = G.split_bf16(A), G.split_bf16(B)
    for m, n in ((0, 0), (5, 4), (2, 3)):
        t = torch.cat([ah[:, m] * bh[:, n], ah[:, m] * bl[:, n], al[:, m] * bh[:, n]]).numpy()
        for seed in (3, 4):
            got = _accumulate_fp32(t, seed)
            assert np.float64(got) == want[m, n].item()
    # the dropped term is visible: more than one fp32 ulp at the largest entry
    full = G.product_tn(A, B, "full")
    lolo = (full - want).abs().max().item()
    ulp = float(np.spacing(np.float32(want.abs().max().item())))
    print(f"[gemm premises] split class K={K}: |C|max {want.abs().max().item():.1f}, lo.lo up to {lolo:.3e} = {lolo / ulp:.1f} ulp")
    assert lolo > ulp


def test_integer_class_premises():
    K = 100001
    assert K <= G.INT_K_MAX and 64 * G.INT_K_MAX < 2 ** 24
    A, qa = G.int_operand(K, 4, 5)
    B, qb = G.int_operand(K, 3, 6)
    for x, q in ((A, qa), (B, qb)):
        hi, lo = G.split_bf16(x)
        assert torch.equal(hi, x) and not lo.any() and torch.equal(x.long(), q)
    want = qa.T @ qb
    assert torch.equal(G.product_tn(A, B, "full"), want.double()) and torch.equal(G.product_tn(A, B, "three"), want.double())
    for m, n in ((0, 0), (3, 2)):
        t = (A[:, m] * B[:, n]).numpy()
        for seed in (7, 8):
            assert int(_accumulate_fp32(t, seed)) == int(want[m, n])


def _loops_nt(A, B, bias, bias_rows, c0, accumulate, relu):
    M, K = A.shape
    N = B.shape[0]
    out = [[0.0] * N for _ in range(M)]
    for m in range(M):
        for n in range(N):
            v = 0.0
            for k in range(K):
                v += float(A[m, k]) * float(B[n, k])
            if bias is not None and m < bias_rows:
                v += float(bias[n])
            if accumulate:
                v += float(c0[m, n])
            out[m][n] = max(v, 0.0) if relu else v
    return torch.tensor(out, dtype=torch.float64)


@pytest.mark.parametrize("cls", ["int", "split"])
def test_reference_against_loops(cls):
    M, N, K = 5, 3, 7
    A, B = G.operand(cls, M, K, 11), G.operand(cls, N, K, 12)
    bias, c0 = G.int_values((N,), 13), G.int_values((M, N), 14)
    for bias_rows, accumulate, relu in itertools.product((0, 2, M), (False, True), (False, True)):
        want = _loops_nt(A, B, bias, bias_rows, c0, accumulate, relu)      # float64 products of fp32 values: exact here
        got = G.ref_nt(A, B, "full", bias if bias_rows else None, bias_rows, c0, accumulate, relu)
        assert torch.equal(got, want), (bias_rows, accumulate, relu)
        if cls == "int":
            assert torch.equal(G.ref_nt(A, B, "three", bias, bias_rows, c0, accumulate, relu), want)
            gi = G.ref_nt_int64(A.long(), B.long(), bias.long(), bias_rows, c0.long(), accumulate, relu)
            assert torch.equal(gi.double(), want)
    # tn with column sums: A [K][M], B [K][N]
    At, Bt = A.T.contiguous(), B.T.contiguous()
    cs0 = G.int_values((M,), 15)
    for rows in (0, 1, K - 1, K):
        Cw, cs = G.ref_tn(At, Bt, c0, "full", cs0, rows)
        assert torch.equal(Cw, _loops_nt(A, B, None, 0, c0, True, False))
        want_cs = torch.tensor([float(cs0[m]) + sum(float(At[r, m]) for r in range(rows)) for m in range(M)], dtype=torch.float64)
        assert torch.equal(cs, want_cs)
    assert G.ref_tn(At, Bt, c0)[1] is None
    if cls == "split":      # three terms = the full product minus lo.lo, by loops
        (ah, al), (bh, bl) = G.split_bf16(A), G.split_bf16(B)
        lolo = _loops_nt(al, bl, None, 0, None, False, False)
        assert torch.equal(G.product_nt(A, B, "three"), G.product_nt(A, B, "full") - lolo)
        assert lolo.abs().max() > 0


def test_layout_helpers():
    x = G.operand("int", 5, 7, 21)
    e = G.Embedded(x, 11, offset=1)
    assert torch.equal(e.view, x) and (e.data_ptr() - e.buf.data_ptr()) % 16 == 4
    flat = e.buf.clone()
    idx = (e.first + torch.arange(5)[:, None] * 11 + torch.arange(7)[None]).reshape(-1)
    assert torch.equal(flat[idx].reshape(5, 7), x)
    flat[idx] = 0.0
    assert int(torch.isnan(flat).sum()) == flat.numel() - 35   # everything but the 35 elements is poison
    c0 = G.int_values((4, 3), 22)
    g = G.GuardedC(c0, 3 + 5 + 14, col0=14)
    assert torch.equal(g.check(), c0)
    g.buf[g.ldc + 13] = 1.0                                  # one float left of the window
    assert not g.sentinels_intact()
    g.reset(c0)
    assert g.sentinels_intact()
    g.buf[(g.M + 1) * g.ldc] = 0.0                           # the guard row after
    assert not g.sentinels_intact()
    v = G.GuardedVec(G.int_values((6,), 23), offset=1)
    assert v.data_ptr() % 16 == 4 and v.check().shape == (6,)


def test_slice_arithmetic():
    # the figures the GPU tests rely on, from the host formulas of csrc/gemm.hip
    assert G.tn_rows_per_block(256, 256, 4000) == (128, 32)             # 32 slices of 128 rows, the last one 32 rows long
    assert G.tn_rows_per_block(256, 256, 100001) == (800, 126)          # the last slice: one row
    assert 100001 - 125 * 800 == 1
    rows, per, mt, nt = G.tiled_rows_per_block([(128, 128), (256, 128), (128, 256), (384, 128), (256, 256)], (700, 300, 1500, 33, 257))
    assert (rows, per, mt, nt) == (256, [3, 2, 6, 1, 2], 3, 2) and sum(per) == 14
    assert G.colsum_row_cases(40, (128,)) == [0, 1, 31, 32, 33, 39, 40]
