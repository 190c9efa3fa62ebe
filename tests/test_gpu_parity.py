"""GPU parity tests: the HIP path (through the C ABI of libclift.so) against the CPU oracle on identical seeded
inputs and against the committed reference-generated golden vectors.

Tolerance (BASELINE.json north_star): 1e-3 relative, fp32.  ``rel_close`` asserts |a-b| <= 1e-3*|b| + 1e-5*max|b|.
Most checks pass a tighter rtol (stated per call).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, T, rel_close, grad_close
from gpu_scenes import DEV, _import, _run_forward_backward, build_model, replay_g12, scene

pytestmark = pytest.mark.gpu


# ============================================================================ GEMM building block
@pytest.mark.parametrize("at,bt", [(0, 0), (0, 1), (1, 1), (1, 0)])
@pytest.mark.parametrize("M,N,K", [(300, 256, 256), (1000, 128, 152), (517, 27, 144), (257, 3, 128), (129, 150, 36), (64, 22, 7)])
def test_gemm_matches_fp64(at, bt, M, N, K):
    from contrastive_lift_amd import engine
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + at * 2 + bt)
    Kp = (K + 3) // 4 * 4
    Mp = (M + 3) // 4 * 4
    Np = (N + 3) // 4 * 4
    A = torch.randn((K, Mp) if at else (M, Kp), generator=g)
    B = torch.randn((K, Np) if bt else (N, Kp), generator=g)
    bias = torch.randn(N, generator=g)
    Aop = A[:, :M].T if at else A[:, :K]
    Bop = B[:, :N].T if bt else B[:, :K]
    ref = Aop.double() @ Bop.double().T + bias.double()
    mask = torch.randn(M, N, generator=g)
    ref_act = torch.relu(ref) * (mask > 0)
    Ad, Bd, biasd, maskd = A.to(DEV), B.to(DEV), bias.to(DEV), mask.to(DEV).contiguous()
    out = torch.full((M, N + 1), -7.0, device=DEV)
    engine.gemm(M, N, K, Ad, A.shape[1], Bd, B.shape[1], out, N + 1, a_trans=at, b_trans=bt, bias=biasd)
    rel_close(out[:, :N], ref, 2e-5, atol=2e-5 * float(ref.abs().max()), what="gemm")
    assert bool((out[:, N] == -7.0).all())           # never writes outside N
    out2 = torch.zeros((M, N), device=DEV)
    engine.gemm(M, N, K, Ad, A.shape[1], Bd, B.shape[1], out2, N, a_trans=at, b_trans=bt, bias=biasd, act=1, mask=maskd, ldmask=N)
    rel_close(out2, ref_act, 2e-5, atol=2e-5 * float(ref.abs().max()), what="gemm relu+mask")
    out3 = torch.ones((M, N), device=DEV)
    engine.gemm(M, N, K, Ad, A.shape[1], Bd, B.shape[1], out3, N, a_trans=at, b_trans=bt, accumulate=1, split_k=3)
    rel_close(out3, ref - bias.double() + 1.0, 2e-5, atol=4e-5 * float(ref.abs().max()), what="gemm split-k accumulate")


@pytest.mark.parametrize("at,bt", [(0, 0), (0, 1), (1, 1), (1, 0)])
@pytest.mark.parametrize("M,N,K", [(300, 256, 256), (1000, 128, 152), (517, 27, 144), (257, 3, 128), (129, 150, 36), (64, 22, 7),
                                   (128 * 3, 256, 64)])
def test_gemm_bf16_mode_matches_rounded_operands(at, bt, M, N, K):
    """bf16 mode (clift_gemm precision = 1): operands rounded to bf16 (RNE) in the kernel, exact products, fp32 accumulate.
    So the result must equal the fp64 product of the bf16-ROUNDED operands to fp32 summation accuracy (2e-5), and the plain
    fp32 product only to bf16 accuracy."""
    from contrastive_lift_amd import engine
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + at * 2 + bt + 1000)
    Kp, Mp, Np = (K + 3) // 4 * 4, (M + 3) // 4 * 4, (N + 3) // 4 * 4
    A = torch.randn((K, Mp) if at else (M, Kp), generator=g)
    B = torch.randn((K, Np) if bt else (N, Kp), generator=g)
    bias = torch.randn(N, generator=g)
    rnd = lambda t: t.to(torch.bfloat16).double()
    Aop = A[:, :M].T if at else A[:, :K]
    Bop = B[:, :N].T if bt else B[:, :K]
    ref = rnd(Aop) @ rnd(Bop).T + bias.double()
    mask = torch.randn(M, N, generator=g)
    Ad, Bd, biasd, maskd = A.to(DEV), B.to(DEV), bias.to(DEV), mask.to(DEV).contiguous()
    prev = engine.set_mlp_precision("bf16")
    try:
        out = torch.full((M, N + 1), -7.0, device=DEV)
        engine.gemm(M, N, K, Ad, A.shape[1], Bd, B.shape[1], out, N + 1, a_trans=at, b_trans=bt, bias=biasd)
        out2 = torch.zeros((M, N), device=DEV)
        engine.gemm(M, N, K, Ad, A.shape[1], Bd, B.shape[1], out2, N, a_trans=at, b_trans=bt, bias=biasd, act=1, mask=maskd, ldmask=N)
        out3 = torch.ones((M, N), device=DEV)
        engine.gemm(M, N, K, Ad, A.shape[1], Bd, B.shape[1], out3, N, a_trans=at, b_trans=bt, accumulate=1, split_k=3)
        colsum = None
        if at:
            colsum = torch.zeros(M, device=DEV)
            out4 = torch.zeros((M, N), device=DEV)
            engine.gemm(M, N, K, Ad, A.shape[1], Bd, B.shape[1], out4, N, a_trans=at, b_trans=bt, accumulate=1, split_k=2, colsum=colsum)
    finally:
        engine.set_mlp_precision(prev)
    scale = float(ref.abs().max())
    rel_close(out[:, :N], ref, 2e-5, atol=2e-5 * scale, what="bf16 gemm vs rounded operands")
    assert bool((out[:, N] == -7.0).all())
    rel_close(out2, torch.relu(ref) * (mask > 0), 2e-5, atol=2e-5 * scale, what="bf16 gemm relu+mask")
    rel_close(out3, ref - bias.double() + 1.0, 2e-5, atol=4e-5 * scale, what="bf16 gemm split-k")
    full = Aop.double() @ Bop.double().T + bias.double()
    assert float((out[:, :N].double().cpu() - full).abs().max()) <= 2e-2 * scale        # bf16-level agreement with fp32 math
    if colsum is not None:
        refc = rnd(Aop).sum(1)
        rel_close(colsum, refc, 1e-4, atol=1e-4 * float(refc.abs().max()) + 1e-5, what="bf16 colsum")


@pytest.mark.parametrize("bt", [0, 1])
@pytest.mark.parametrize("M,N,K", [(300, 256, 256), (1000, 128, 152), (517, 27, 144), (257, 3, 128), (129, 150, 36), (64, 22, 7),
                                   (128 * 5 + 1, 256, 64)])
def test_gemm_fp32x6_split_is_fp32_faithful(bt, M, N, K):
    """fp32x6 (clift_gemm precision = 2): every operand split exactly into three bf16 terms, six products on the bf16 matrix
    cores, fp32 accumulate.  It must meet the SAME fp64 tolerance as the exact-fp32 kernel (2e-5 of the tensor scale), and its
    worst error must stay within 4x of the exact-fp32 kernel's own round-off on the same problem."""
    from contrastive_lift_amd import engine
    g = torch.Generator().manual_seed(M * 5 + N * 3 + K + bt + 77)
    Kp, Np = (K + 3) // 4 * 4, (N + 3) // 4 * 4
    A = torch.randn((M, Kp), generator=g) * torch.exp(2.0 * torch.randn((M, 1), generator=g))      # rows of very different scale
    B = torch.randn((K, Np) if bt else (N, Kp), generator=g)
    bias = torch.randn(N, generator=g)
    Bop = B[:, :N].T if bt else B[:, :K]
    ref = A[:, :K].double() @ Bop.double().T + bias.double()
    mask = torch.randn(M, N, generator=g)
    Ad, Bd, biasd, maskd = A.to(DEV), B.to(DEV), bias.to(DEV), mask.to(DEV).contiguous()
    outs = {}
    for mode in ("fp32", "fp32x6"):
        prev = engine.set_mlp_precision(mode)
        try:
            o1 = torch.full((M, N + 1), -7.0, device=DEV)
            engine.gemm(M, N, K, Ad, A.shape[1], Bd, B.shape[1], o1, N + 1, b_trans=bt, bias=biasd)
            o2 = torch.zeros((M, N), device=DEV)
            engine.gemm(M, N, K, Ad, A.shape[1], Bd, B.shape[1], o2, N, b_trans=bt, bias=biasd, act=1, mask=maskd, ldmask=N)
        finally:
            engine.set_mlp_precision(prev)
        outs[mode] = (o1, o2)
    row_scale = ref.abs().amax(1, keepdim=True).clamp_min(1e-30)
    err = {k: float(((v[0][:, :N].double().cpu() - ref).abs() / row_scale).max()) for k, v in outs.items()}
    assert bool((outs["fp32x6"][0][:, N] == -7.0).all())
    assert err["fp32x6"] <= 2e-5, err
    assert err["fp32x6"] <= 4.0 * err["fp32"] + 2e-7, err                 # same order as fp32 round-off, row by row
    rel_close(outs["fp32x6"][1], torch.relu(ref) * (mask > 0), 2e-5, atol=2e-5 * float(ref.abs().max()), what="fp32x6 relu+mask")


@pytest.mark.parametrize("M,N,K", [(300, 256, 256), (1000, 128, 152), (517, 24, 256), (130, 256, 24), (128 * 3 + 5, 256, 64)])
def test_gemm_bf16_stored_operands(M, N, K):
    """bf16 mode with bf16-STORED tensors (hidden activations / gradients): forward with A and C stored as bf16, dgrad with a
    bf16 mask and bf16 output, wgrad with both streamed operands stored as bf16 -- against fp64 products of the same bf16
    values (outputs compared after their own bf16 rounding where they are bf16-stored)."""
    from contrastive_lift_amd import engine
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K)
    bf = torch.bfloat16
    Kp, Np = (K + 7) // 8 * 8, (N + 7) // 8 * 8
    A = torch.randn((M, Kp), generator=g).to(bf)
    W = torch.randn((N, (K + 3) // 4 * 4), generator=g)                     # weights stay fp32 (rounded in-kernel)
    bias = torch.randn(N, generator=g)
    Wr = W[:, :K].to(bf).double()
    ref = A[:, :K].double() @ Wr.T + bias.double()
    prev = engine.set_mlp_precision("bf16")
    try:
        Ad, Wd, bd = A.to(DEV), W.to(DEV), bias.to(DEV)
        out = torch.zeros((M, Np), dtype=bf, device=DEV)
        engine.gemm(M, N, K, Ad, Kp, Wd, W.shape[1], out, Np, bias=bd, act=1)                       # fwd: bf16 A -> bf16 C, ReLU
        want = torch.relu(ref)
        got = out[:, :N].double().cpu()
        assert float((got - want).abs().max()) <= 1.0 / 128 * float(want.abs().max()) + 1e-6          # one bf16 rounding of the output
        out32 = torch.zeros((M, N), device=DEV)
        engine.gemm(M, N, K, Ad, Kp, Wd, W.shape[1], out32, N, bias=bd)                               # fwd: bf16 A -> fp32 C
        rel_close(out32, ref, 2e-5, atol=2e-5 * float(ref.abs().max()), what="bf16-stored A, fp32 C")
        # dgrad: dX (M,K) = (dY (M,N) bf16) W, masked by a bf16 activation, bf16 output
        dY = torch.randn((M, Np), generator=g).to(bf)
        mask = torch.relu(torch.randn((M, Kp), generator=g)).to(bf)
        dX = torch.zeros((M, Kp), dtype=bf, device=DEV)
        engine.gemm(M, K, N, dY.to(DEV), Np, Wd, W.shape[1], dX, Kp, b_trans=1, mask=mask.to(DEV), ldmask=Kp)
        refd = (dY[:, :N].double() @ W[:, :K].to(bf).double()) * (mask[:, :K].double() > 0)
        assert float((dX[:, :K].double().cpu() - refd).abs().max()) <= 1.0 / 128 * float(refd.abs().max()) + 1e-6
        # wgrad: dW (N,K) += dY^T A, both streamed operands bf16-stored, fp32 accumulate + fused bias sums
        gW = torch.zeros((N, (K + 3) // 4 * 4), device=DEV)
        gb = torch.zeros(N, device=DEV)
        if N > 32:
            engine.wgrad(N, K, M, dY.to(DEV), Np, Ad, Kp, gW, gb)
            refw = dY[:, :N].double().T @ A[:, :K].double()
            rel_close(gW[:, :K], refw, 1e-4, atol=1e-4 * float(refw.abs().max()), what="wgrad bf16-stored operands")
            rel_close(gb, dY[:, :N].double().sum(0), 1e-4, atol=1e-4 * M ** 0.5, what="bias sums")
    finally:
        engine.set_mlp_precision(prev)


@pytest.mark.parametrize("M", [4096, 4097, 8191, 40000, 249001])
def test_persistent_fp32_hidden_layer(M):
    """layer_f32.hip (exact fp32; persistent blocks, weights in registers, LDS-DMA row stream, bias as an extra MFMA step): the
    256 -> 256 forward with and without bias / ReLU against fp64, every row of ragged ranges; rows beyond M and the pad column
    untouched; and bit-for-bit the same sums as the tiled kernel up to summation order (2e-6 relative to the row scale)."""
    from contrastive_lift_amd import engine
    g = torch.Generator().manual_seed(M + 5)
    A = torch.randn((M, 256), generator=g)
    W = (torch.randn((256, 256), generator=g) / 16).contiguous()
    bias = torch.randn(256, generator=g)
    ref = A.double() @ W.double().T + bias.double()
    Ad, Wd, bd = A.to(DEV), W.to(DEV), bias.to(DEV)
    out = torch.full((M + 2, 260), -7.0, device=DEV)
    engine.gemm(M, 256, 256, Ad, 256, Wd, 256, out, 260, bias=bd, act=1)
    rel_close(out[:M, :256], torch.relu(ref), 2e-5, atol=2e-5 * float(ref.abs().max()), what="persistent fp32 layer, bias + relu")
    assert bool((out[M:] == -7.0).all()) and bool((out[:, 256:] == -7.0).all())
    out2 = torch.zeros((M, 256), device=DEV)
    engine.gemm(M, 256, 256, Ad, 256, Wd, 256, out2, 256)
    rel_close(out2, ref - bias.double(), 2e-5, atol=2e-5 * float(ref.abs().max()), what="persistent fp32 layer, plain")
    with engine.kernel_switches(tiled_only=True):          # the tiled kernel on the same inputs
        out3 = torch.zeros((M, 256), device=DEV)
        engine.gemm(M, 256, 256, Ad, 256, Wd, 256, out3, 256)
    scale = (A.abs().double() @ W.abs().double().T).to(DEV)
    assert float(((out2 - out3).abs().double() / scale).max()) <= 2e-6
    # masked dgrad of the same layer (k_layer_f32_dgrad): dX = mask . (dY W), W read along its rows
    mask = torch.randn((M, 256), generator=g)
    maskd = mask.to(DEV)
    dX = torch.full((M + 2, 260), -7.0, device=DEV)
    engine.gemm(M, 256, 256, Ad, 256, Wd, 256, dX, 260, b_trans=1, mask=maskd, ldmask=256)
    refd = (A.double() @ W.double()) * (mask.double() > 0)
    rel_close(dX[:M, :256], refd, 2e-5, atol=2e-5 * float(refd.abs().max()), what="persistent fp32 dgrad")
    assert bool((dX[M:] == -7.0).all()) and bool((dX[:, 256:] == -7.0).all())
    assert bool((dX[:M, :256][maskd <= 0] == 0).all())


@pytest.mark.parametrize("M", [64, 65, 97, 300, 8191, 33000, 174001])
def test_streamed_bf16_hidden_layer(M):
    """layer_bf16.hip (persistent blocks, weights in registers, LDS-DMA ring, counted waits): the 256 -> 256 forward (bias + ReLU)
    and masked dgrad with bf16-stored tensors, element by element against fp64 products of the same bf16 values -- every row of
    ragged row ranges, tile boundaries and multi-tile blocks; rows beyond M and the pad columns stay untouched."""
    from contrastive_lift_amd import engine
    g = torch.Generator().manual_seed(M)
    bf = torch.bfloat16
    A = torch.randn((M, 256), generator=g).to(bf)
    W = (torch.randn((256, 256), generator=g) / 16).contiguous()
    bias = torch.randn(256, generator=g)
    Wr = W.to(bf).double()
    prev = engine.set_mlp_precision("bf16")
    try:
        Ad, Wd = A.to(DEV), W.to(DEV)
        out = torch.full((M + 3, 256), -7.0, dtype=bf, device=DEV)
        engine.gemm(M, 256, 256, Ad, 256, Wd, 256, out, 256, bias=bias.to(DEV), act=1)
        want = torch.relu(A.double() @ Wr.T + bias.double())
        got = out[:M].double().cpu()
        tol = want.abs() / 256 + 2e-5 * float(want.abs().max())               # one bf16 rounding of the output + summation order
        assert bool(((got - want).abs() <= tol).all()), float(((got - want).abs() - tol).max())
        assert bool((out[M:] == -7.0).all())
        dY = torch.randn((M, 256), generator=g).to(bf)
        mask = torch.relu(torch.randn((M, 256), generator=g)).to(bf)
        dX = torch.full((M + 3, 256), -7.0, dtype=bf, device=DEV)
        engine.gemm(M, 256, 256, dY.to(DEV), 256, Wd, 256, dX, 256, b_trans=1, mask=mask.to(DEV), ldmask=256)
        wantd = (dY.double() @ Wr) * (mask.double() > 0)
        gotd = dX[:M].double().cpu()
        told = wantd.abs() / 256 + 2e-5 * float(wantd.abs().max())
        assert bool(((gotd - wantd).abs() <= told).all()), float(((gotd - wantd).abs() - told).max())
        assert bool((dX[M:] == -7.0).all())
        assert bool((gotd[mask.double() <= 0] == 0).all())
    finally:
        engine.set_mlp_precision(prev)


@pytest.mark.parametrize("M", [64, 65, 200, 4096, 70001, 174001])
def test_streamed_bf16_weight_gradient(M):
    """k_wgrad_bf16_stream (persistent blocks, both operands by LDS-DMA, ds_read_b64_tr_b16 fragments): gW += dY^T X and the fused
    bias sums for the 256 x 256 layers with bf16-stored operands, against fp64 on the same bf16 values; accumulates onto existing
    contents; ragged row counts (zero-filled last tile)."""
    from contrastive_lift_amd import engine
    g = torch.Generator().manual_seed(M + 11)
    bf = torch.bfloat16
    dY = torch.randn((M, 256), generator=g).to(bf)
    X = torch.relu(torch.randn((M, 256), generator=g)).to(bf)
    prev = engine.set_mlp_precision("bf16")
    try:
        gW = torch.full((256, 256), 0.5, device=DEV)
        gb = torch.full((256,), -2.0, device=DEV)
        engine.wgrad(256, 256, M, dY.to(DEV), 256, X.to(DEV), 256, gW, gb)
        refw = dY.double().T @ X.double() + 0.5
        refb = dY.double().sum(0) - 2.0
        rel_close(gW, refw, 1e-4, atol=1e-4 * float(refw.abs().max()), what="streamed wgrad")
        rel_close(gb, refb, 1e-4, atol=1e-4 * M ** 0.5, what="streamed bias sums")
    finally:
        engine.set_mlp_precision(prev)


@pytest.mark.parametrize("xb", [False, True])
@pytest.mark.parametrize("M,no,ldd", [(4096, 22, 24), (4099, 3, 4), (40001, 22, 24), (249003, 3, 4), (5000, 32, 32), (8191, 6, 8)])
def test_narrow_wgrad_stream(M, no, ldd, xb):
    """k_wgrad_narrow_stream (output-layer weight gradients on the fp32 matrix cores, X streamed by LDS-DMA; fp32 or bf16-stored X):
    gW += dY^T X and gb += column sums against fp64, accumulating onto existing contents, ragged row counts, zero pad columns of
    dY ignored; and the same numbers as the VALU kernel it replaces."""
    from contrastive_lift_amd import engine
    g = torch.Generator().manual_seed(M + no)
    dY = torch.zeros((M, ldd))
    dY[:, :no] = torch.randn((M, no), generator=g)
    X = torch.relu(torch.randn((M, 256), generator=g))
    if xb:
        X = X.to(torch.bfloat16)
    prev = engine.set_mlp_precision("bf16" if xb else "fp32")
    try:
        gW = torch.full((no, 256), 0.25, device=DEV)
        gb = torch.full((no,), -1.0, device=DEV)
        engine.wgrad(no, 256, M, dY.to(DEV), ldd, X.to(DEV), 256, gW, gb)
        refw = dY[:, :no].double().T @ X.double() + 0.25
        refb = dY[:, :no].double().sum(0) - 1.0
        rel_close(gW, refw, 2e-5, atol=2e-5 * float(refw.abs().max()), what="narrow wgrad (stream)")
        rel_close(gb, refb, 2e-5, atol=2e-5 * M ** 0.5, what="narrow bias sums (stream)")
        with engine.kernel_switches(tiled_only=True):
            gW2 = torch.full((no, 256), 0.25, device=DEV)
            gb2 = torch.full((no,), -1.0, device=DEV)
            engine.wgrad(no, 256, M, dY.to(DEV), ldd, X.to(DEV), 256, gW2, gb2)
        rel_close(gW, gW2, 2e-5, atol=2e-5 * float(refw.abs().max()), what="stream vs VALU kernel")
    finally:
        engine.set_mlp_precision(prev)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("M,K,lda", [(4096, 22, 24), (4101, 3, 4), (60001, 22, 24), (249003, 3, 4), (5000, 32, 32), (8191, 6, 8)])
def test_narrow_dgrad_stream(M, K, lda, half):
    """k_dgrad_narrow_stream (first step of the hidden-layer backward: dX = mask . (dOut W) for the 22-class / 3-dim output layers,
    fp32 or bf16-stored mask and result): every row of ragged row counts against fp64; rows beyond M and pad columns untouched."""
    from contrastive_lift_amd import engine
    g = torch.Generator().manual_seed(M + K)
    bf = torch.bfloat16
    dO = torch.zeros((M, lda))
    dO[:, :K] = torch.randn((M, K), generator=g)
    W = torch.randn((K, 256), generator=g)
    mask = torch.relu(torch.randn((M, 256), generator=g))
    ref = (dO[:, :K].double() @ W.double()) * (mask.double() > 0)
    prev = engine.set_mlp_precision("bf16" if half else "fp32")
    try:
        md = mask.to(bf).to(DEV) if half else mask.to(DEV)
        refm = ref if not half else (dO[:, :K].double() @ W.double()) * (mask.to(bf).double() > 0)
        dX = torch.full((M + 2, 260), -7.0, dtype=bf if half else torch.float32, device=DEV)
        engine.gemm(M, 256, K, dO.to(DEV), lda, W.to(DEV), 256, dX, 260, b_trans=1, mask=md, ldmask=256)
        got = dX[:M, :256].double().cpu()
        if half:   # the tiled bf16 kernel rounds both operands to bf16 first; this kernel multiplies in fp32 and rounds the result once
            tol = refm.abs() / 128 + 1e-2 * float(refm.abs().max()) / 128
            assert bool(((got - refm).abs() <= tol).all()), float(((got - refm).abs() - tol).max())
        else:
            rel_close(got, refm, 2e-5, atol=2e-5 * float(refm.abs().max()), what="narrow dgrad (stream)")
        assert bool((dX[M:] == -7.0).all()) and bool((dX[:, 256:] == -7.0).all())
        assert bool((got[(mask.to(bf) if half else mask).double() <= 0] == 0).all())
    finally:
        engine.set_mlp_precision(prev)


@pytest.mark.parametrize("M,Nout", [(1, 256), (5, 256), (8191, 256), (100003, 256), (40001, 128), (3001, 24), (777, 4)])
def test_linear_k3_forward(M, Nout):
    """clift_linear_k3_fwd (first layer of the xyz heads, tensoRF.py:475,576): every row and column against torch, with and without
    ReLU, fp32 and bf16-stored output, rows beyond M untouched; widths whose column-quad count does not divide 256 take the
    generic kernel."""
    from contrastive_lift_amd import _lib
    g = torch.Generator().manual_seed(M + Nout)
    x = torch.randn((M, 4), generator=g)
    W = torch.randn((Nout, 4), generator=g)           # pitch 4, three weights used
    b = torch.randn(Nout, generator=g)
    ref = x[:, :3].double() @ W[:, :3].double().T + b.double()
    xd, Wd, bd = x.to(DEV), W.to(DEV), b.to(DEV)
    for relu in (0, 1):
        want = torch.relu(ref) if relu else ref
        out = torch.full((M + 1, Nout + 4), -7.0, device=DEV)
        _lib.call("clift_linear_k3_fwd", _lib.ptr(xd), _lib.ptr(Wd), 4, _lib.ptr(bd), M, Nout, relu, _lib.ptr(out), Nout + 4, 0, _lib.stream())
        rel_close(out[:M, :Nout], want, 1e-5, atol=1e-5 * float(ref.abs().max()), what="k3 fwd")
        assert bool((out[M:] == -7.0).all()) and bool((out[:, Nout:] == -7.0).all())
        outh = torch.full((M + 1, Nout + 4), -7.0, dtype=torch.bfloat16, device=DEV)
        _lib.call("clift_linear_k3_fwd", _lib.ptr(xd), _lib.ptr(Wd), 4, _lib.ptr(bd), M, Nout, relu, _lib.ptr(outh), Nout + 4, 1, _lib.stream())
        goth = outh[:M, :Nout].double().cpu()
        assert bool(((goth - want).abs() <= want.abs() / 256 + 1e-5 * float(ref.abs().max())).all())
        assert bool((outh[M:] == -7.0).all()) and bool((outh[:, Nout:] == -7.0).all())


@pytest.mark.parametrize("hb", [False, True])
@pytest.mark.parametrize("M", [4096, 4100, 40001, 249003, 300])
def test_linear_k3_backward(M, hb):
    """clift_linear_k3_bwd (dW[n][0..2] += sum_m dH[m][n] x[m][:], db[n] += sum_m dH[m][n]; for M >= 4096 the matrix-core stream of
    narrow_stream.hip with the bias as a forced-ones class, below that the VALU kernel): against fp64, accumulating onto existing
    contents, fp32 and bf16-stored dH, ragged row counts, whatever the pad component of x holds."""
    from contrastive_lift_amd import _lib
    g = torch.Generator().manual_seed(M + 17)
    x = torch.randn((M, 4), generator=g)              # the 4th component is padding: it must not matter
    dH = torch.randn((M, 256), generator=g)
    if hb:
        dH = dH.to(torch.bfloat16)
    dW = torch.full((256, 4), 0.5, device=DEV)
    db = torch.full((256,), -1.5, device=DEV)
    xd, dHd = x.to(DEV), dH.to(DEV)                    # (named: a temporary would be recycled by the allocator before the launch)
    _lib.call("clift_linear_k3_bwd", _lib.ptr(xd), _lib.ptr(dHd), 256, M, 256, _lib.ptr(dW), 4, _lib.ptr(db), int(hb), _lib.stream())
    torch.cuda.synchronize()
    refw = dH.double().T @ x[:, :3].double() + 0.5
    refb = dH.double().sum(0) - 1.5
    rel_close(dW[:, :3], refw, 2e-5, atol=2e-5 * float(refw.abs().max()), what="k3 bwd dW")
    rel_close(db, refb, 2e-5, atol=2e-5 * M ** 0.5, what="k3 bwd db")
    assert bool((dW[:, 3] == 0.5).all())


@pytest.mark.parametrize("M", [4096, 4100, 70001, 159003])
def test_persistent_fp32_weight_gradient(M):
    """k_wgrad_f32_stream (64 row ranges x 4 column slices, LDS-DMA ring): gW += dY^T X and the fused bias sums of the 256 x 256 layers
    against fp64, accumulating onto existing contents, ragged row counts; and the same numbers as the split-K tiled launch."""
    from contrastive_lift_amd import engine
    g = torch.Generator().manual_seed(M + 29)
    dY = torch.randn((M, 256), generator=g)
    X = torch.relu(torch.randn((M, 256), generator=g))
    dYd, Xd = dY.to(DEV), X.to(DEV)
    gW = torch.full((256, 256), 0.5, device=DEV)
    gb = torch.full((256,), -2.0, device=DEV)
    engine.wgrad(256, 256, M, dYd, 256, Xd, 256, gW, gb)
    refw = dY.double().T @ X.double() + 0.5
    refb = dY.double().sum(0) - 2.0
    rel_close(gW, refw, 2e-5, atol=2e-5 * float(refw.abs().max()), what="persistent wgrad")
    rel_close(gb, refb, 2e-5, atol=2e-5 * M ** 0.5, what="persistent wgrad bias sums")
    with engine.kernel_switches(tiled_only=True):
        gW2 = torch.full((256, 256), 0.5, device=DEV)
        gb2 = torch.full((256,), -2.0, device=DEV)
        engine.wgrad(256, 256, M, dYd, 256, Xd, 256, gW2, gb2)
    rel_close(gW, gW2, 2e-5, atol=2e-5 * float(refw.abs().max()), what="persistent vs tiled wgrad")


def test_gemm_tail_split_ctrans_colsum():
    """Large-M launch that takes the main + small-tile remainder path; transposed-output and fused bias-sum modes."""
    from contrastive_lift_amd import engine
    g = torch.Generator().manual_seed(5)
    M, N, K = 128 * 547 + 77, 256, 64                      # 548 row tiles -> 1 full round of 512 + remainder
    A = torch.randn((M, K), generator=g).to(DEV)
    B = torch.randn((N, K), generator=g).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    mask = torch.randn((M, N), generator=g).to(DEV)
    out = torch.empty((M, N), device=DEV)
    engine.gemm(M, N, K, A, K, B, K, out, N, bias=bias, act=1, mask=mask, ldmask=N)
    ref = torch.relu(A.double() @ B.double().T + bias.double()) * (mask > 0)
    rel_close(out, ref, 2e-5, atol=2e-5 * float(ref.abs().max()), what="tail-split gemm")
    # wgrad forms: dW (no x ni) = dY^T X, with fused column sums (wide) and via the transposed problem (narrow)
    Ms = 40000
    for no, ni in ((256, 256), (128, 152), (22, 256), (3, 128), (27, 144)):
        ldd = (no + 3) // 4 * 4
        dY = torch.zeros((Ms, ldd), device=DEV); dY[:, :no] = torch.randn((Ms, no), generator=g).to(DEV)
        X = torch.randn((Ms, ni), generator=g).to(DEV)
        gW = torch.zeros((no, ni), device=DEV); gb = torch.zeros(no, device=DEV)
        engine.wgrad(no, ni, Ms, dY, ldd, X, ni, gW, gb)
        refW = dY[:, :no].double().T @ X.double()
        rel_close(gW, refW, 1e-4, atol=1e-4 * float(refW.abs().max()), what=f"wgrad {no}x{ni}")
        refb = dY[:, :no].double().sum(0)
        rel_close(gb, refb, 1e-4, atol=1e-4 * float(refb.abs().max()) + 1e-4, what=f"bias grad {no}")


def test_gemm_transpose_detecting():
    """A = I against an asymmetric B: a swapped C-write would pass a symmetric test."""
    from contrastive_lift_amd import engine
    n = 64
    A = torch.eye(n, device=DEV)
    B = (torch.arange(n * n, dtype=torch.float32, device=DEV).reshape(n, n) / 100).contiguous()
    out = torch.empty((n, n), device=DEV)
    engine.gemm(n, n, n, A, n, B, n, out, n)
    assert torch.equal(out, B.T.contiguous())


# ============================================================================ ray generation (a1-a3)
def test_gen_rays_golden():
    cl, *_ = _import()
    g = load_golden("g1_rays")
    rays = cl.generate_ray_table(int(g["H"]), int(g["W"]), g["K"], g["c2w"])
    rel_close(rays[:, 0:3], g["o"], 1e-6, what="o")
    rel_close(rays[:, 3:6], g["d"], 1e-5, what="d")
    rel_close(rays[:, 7], g["far"], 1e-5, what="far")
    assert float((rays[:, 6] - 0.01).abs().max()) == 0.0
    with pytest.raises(AssertionError):
        c2w = np.eye(4, dtype=np.float32); c2w[:3, 3] = [0, 0, -3.0]
        cl.generate_ray_table(4, 4, np.array([[1e-3, 0, 2], [0, 1e-3, 2], [0, 0, 1]], np.float32), c2w)


# ============================================================================ sampling / density / weights (a4-a8)
@pytest.mark.parametrize("case", ["tiny_jitter", "tiny_plain", "mid"])
def test_density_and_weights_vs_oracle(case):
    cl, op, orender, ofld, olosses, orays = _import()
    if case == "mid":
        res, n_rays, aabb = (40, 48, 56), 700, torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])
    else:
        res, n_rays, aabb = (9, 13, 17), 130, torch.tensor([[-0.9, -0.7, -0.5], [0.8, 0.7, 0.6]])
    P, rays, rng = scene(op, orays, 11, res, 3, 3, n_rays)
    rays[0, 3:6] = torch.tensor([0.0, 0.0, 1.0])
    rays[1, 0:3] = 0.0
    jitter = None if case == "tiny_plain" else torch.from_numpy(rng.uniform(0, 1, n_rays).astype(np.float32))
    cfg = orender.RenderCfg(aabb, res, density_shift=-3.0)
    with torch.no_grad():
        (_, _, _, depth, _, dreg), aux = orender.render_forward(P, rays, cfg, jitter, False, return_aux=True)
    from contrastive_lift_amd import engine
    m = build_model(cl, P, res, 3, 3, -3.0)
    r = cl.TensoRFRenderer(aabb, list(res), semantic_weight_mode="softmax").to(DEV)
    assert r.n_samples == cfg.n_samples
    ctx = engine._density_march(m, r, rays.to(DEV), None if jitter is None else jitter.to(DEV))
    rel_close(ctx.w, aux["w"], 1e-4, atol=1e-7, what="weights")
    rel_close(ctx.alpha, aux["alpha"], 1e-4, atol=2e-7, what="alpha")
    rel_close(ctx.ray_out[:, 0], aux["opacity"], 1e-4, what="opacity")
    rel_close(ctx.ray_out[:, 1], depth, 1e-4, what="depth")
    rel_close(ctx.ray_out[:, 2], aux["bg"][:, 0], 1e-4, atol=1e-7, what="bg")
    rel_close(ctx.ray_out[:, 5].mean(), dreg, 1e-4, what="dist_reg (unpinned formula)")
    # the compacted list is exactly the oracle's active mask (threshold flips allowed only within 1e-7 of it)
    act = torch.zeros(ctx.N * ctx.S, dtype=torch.bool)
    act[ctx.act_idx[:ctx.M].cpu().long()] = True
    diff = act.view(ctx.N, ctx.S) != aux["active"]
    assert int(diff.sum()) == 0 or float((aux["w"][diff] - 1e-4).abs().max()) < 1e-7
    assert bool((ctx.act_idx[:ctx.M][1:] > ctx.act_idx[:ctx.M][:-1]).all())       # sorted = ray-major, k ascending


# ============================================================================ full forward + backward (a9-a13)
@pytest.mark.parametrize("mode", ["softmax", "none", "argmax"])
@pytest.mark.parametrize("white", [False, True])
def test_forward_backward_golden_g6(mode, white):
    """Against the reference's own outputs and gradients (tests/golden/g6_forward.npz; g6a_forward_argmax.npz for R:142-143's one-hot weights)."""
    cl, op, *_ = _import()
    g = load_golden("g6a_forward_argmax" if mode == "argmax" else "g6_forward")
    res = tuple(int(x) for x in g["res"])
    C_, E = int(g["C"]), int(g["E"])
    P = op.add_blob(op.make_params(int(g["seed"]), res, C_, E), res, 2.5, 0.45)
    m = build_model(cl, P, res, C_, E, float(g["shift"]), mode)
    r = cl.TensoRFRenderer(T(g["aabb"]), list(res), semantic_weight_mode=mode).to(DEV)
    tag = f"{mode}_{'w' if white else 'b'}"
    outs, grads = _run_forward_backward(cl, m, r, T(g["rays"]), T(g["jitter"]), white, (T(g["cot_rgb"]), T(g["cot_sem"]), T(g["cot_inst"])))
    rel_close(outs[0], g[f"{tag}.rgb"], 1e-3, what="rgb")
    rel_close(outs[1], g[f"{tag}.sem"], 1e-3, what="sem")
    rel_close(outs[2], g[f"{tag}.inst"], 1e-3, what="inst")
    rel_close(outs[3], g[f"{tag}.depth"], 1e-3, what="depth")
    assert tuple(outs[4].shape) == (1, 1)
    n = 0
    for k, gr in grads.items():
        key = f"{tag}.gsub.{k}"
        if key not in g:
            continue
        flat = gr.detach().reshape(-1) if gr is not None else torch.zeros(1)
        if gr is not None and gr.dim() == 4:    # channels-last view -> logical NCHW order of the fixture
            flat = gr.detach().contiguous(memory_format=torch.contiguous_format).reshape(-1)
        elif gr is not None:
            flat = gr.detach().contiguous().reshape(-1)
        sub = flat if flat.numel() <= 4096 else flat[::17]
        ref = T(g[key]).double()
        scale = float(T(g[f"{tag}.gnorm.{k}"])) / max(1.0, np.sqrt(flat.numel()))
        rel_close(sub, ref, 2e-3, atol=2e-3 * max(scale, 1e-12) + 1e-9, what=key)
        rel_close(flat.norm(), g[f"{tag}.gnorm.{k}"], 1e-3, atol=1e-9, what=f"norm {k}")
        n += 1
    assert n >= 30


@pytest.mark.parametrize("mode,white", [("softmax", False), ("none", True), ("argmax", True)])
def test_forward_backward_vs_oracle_mid(mode, white):
    """A larger anisotropic scene (grid 40x48x56, 900 rays, C=22) including the dist-reg gradient path."""
    cl, op, orender, ofld, olosses, orays = _import()
    res, C_, E, n_rays = (40, 48, 56), 22, 3, 900
    aabb = torch.tensor([[-0.9, -0.8, -0.7], [0.8, 0.9, 0.75]])
    P, rays, rng = scene(op, orays, 23, res, C_, E, n_rays, amp=2.2, sg=0.4)
    jitter = torch.from_numpy(rng.uniform(0, 1, n_rays).astype(np.float32))
    cots = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)) for s in ((n_rays, 3), (n_rays, C_), (n_rays, 2 * E))]
    Pg = op.clone_params(P, requires_grad=True)
    cfg = orender.RenderCfg(aabb, res, density_shift=-3.0, semantic_weight_mode=mode)
    o = orender.render_forward(Pg, rays, cfg, jitter, white)
    L = (o[0] * cots[0]).sum() + (o[1] * cots[1]).sum() + (o[2] * cots[2]).sum() + 3.0 * o[5]
    L.backward()
    m = build_model(cl, P, res, C_, E, -3.0, mode)
    r = cl.TensoRFRenderer(aabb, list(res), semantic_weight_mode=mode).to(DEV)
    outs, grads = _run_forward_backward(cl, m, r, rays, jitter, white, cots + [3.0])
    for a, b, nm in zip(outs[:4], o[:4], ("rgb", "sem", "inst", "depth")):
        rel_close(a, b.detach(), 1e-3, what=nm)
    rel_close(outs[5], o[5].detach(), 1e-3, what="dist_reg")
    for k, gr in grads.items():
        ref = Pg[k].grad
        ref = torch.zeros_like(Pg[k]) if ref is None else ref
        got = torch.zeros_like(ref) if gr is None else gr.detach().cpu()
        # 2e-3 relative + 1e-4 of the tensor's scale for all but <= 0.1 % of the entries, and those within 1e-3 of the scale: a hidden
        # unit whose pre-activation is zero to round-off for one sample lands on either side of the ReLU kink depending on the
        # summation order of the layer before it, which moves one row of the next weight gradient by that sample's contribution
        # (observed: one row of one 256 x 256 gradient differs by 4e-4 of its scale between the tiled and the persistent forward
        # kernel, everything else to 1e-6)
        # (table gradients: one such sample touches 2 line texels x 16 / 48 channels per plane, i.e. ~10 entries of a 2688-entry line
        # table at once
        # table entries at once -- hence the 0.5 % allowance there, 1 % for the 27 x 144 basis matrix right behind the tables)
        grad_close(got, ref, what=f"grad {k}", rtol=2e-3, scale_atol=1e-4,
                   outlier_frac=(5e-3 if k.split(".")[0].endswith(("_plane", "_line")) else 1e-2 if k.startswith("appearance_basis") else 1e-3),
                   outlier_cap=1e-3)


def test_forward_backward_vs_oracle_large_grid_no_lds_lines():
    """Grid 300 x 280 x 330 (beyond the reference's 192^3): the appearance line accumulators (910 x 48 floats = 175 KB) no
    longer fit the 160 KB LDS, so k_app_gather_bwd takes its global-atomic line path (LDS_LINES = false) while the density
    kernel (58 KB) keeps the LDS path; also covers XCD-private accumulation copies at a large table size."""
    cl, op, orender, ofld, olosses, orays = _import()
    res, C_, E, n_rays = (300, 280, 330), 5, 3, 96
    aabb = torch.tensor([[-0.9, -0.8, -0.7], [0.8, 0.9, 0.75]])
    P, rays, rng = scene(op, orays, 29, res, C_, E, n_rays, amp=2.2, sg=0.4)
    jitter = torch.from_numpy(rng.uniform(0, 1, n_rays).astype(np.float32))
    cots = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)) for s in ((n_rays, 3), (n_rays, C_), (n_rays, 2 * E))]
    Pg = op.clone_params(P, requires_grad=True)
    cfg = orender.RenderCfg(aabb, res, density_shift=-3.0, semantic_weight_mode="softmax")
    o = orender.render_forward(Pg, rays, cfg, jitter, False)
    L = (o[0] * cots[0]).sum() + (o[1] * cots[1]).sum() + (o[2] * cots[2]).sum() + 3.0 * o[5]
    L.backward()
    m = build_model(cl, P, res, C_, E, -3.0, "softmax")
    r = cl.TensoRFRenderer(aabb, list(res), semantic_weight_mode="softmax").to(DEV)
    outs, grads = _run_forward_backward(cl, m, r, rays, jitter, False, cots + [3.0])
    for a, b, nm in zip(outs[:4], o[:4], ("rgb", "sem", "inst", "depth")):
        rel_close(a, b.detach(), 1e-3, what=nm)
    for k in ("density_plane.0", "density_line.2", "appearance_plane.1", "appearance_line.0", "appearance_line.1", "appearance_line.2"):
        ref = Pg[k].grad
        got = grads[k].detach().cpu()
        rel_close(got, ref, 2e-3, atol=2e-3 * float(ref.abs().max()) * 0.05 + 1e-10, what=f"grad {k}")


def test_instance_and_segment_golden_g7():
    cl, op, *_ = _import()
    g = load_golden("g7_instance_segment")
    res = tuple(int(x) for x in g["res"])
    C_, E = int(g["C"]), int(g["E"])
    P = op.add_blob(op.make_params(int(g["seed"]), res, C_, E), res, 2.5, 0.45)
    m = build_model(cl, P, res, C_, E, float(g["shift"]))
    r = cl.TensoRFRenderer(T(g["aabb"]), list(res), semantic_weight_mode="softmax").to(DEV)
    rays = T(g["rays"]).to(DEV)
    inst, xyz = r.forward_instance_feature(m, rays, 0, False)
    rel_close(inst, g["inst"], 1e-3, what="inst")
    rel_close(xyz, g["xyz"], 1e-3, what="xyz")
    grads = torch.autograd.grad((inst * T(g["cot_inst"]).to(DEV)).sum(), list(m.parameters()), allow_unused=True)
    n = 0
    for (k, _), gr in zip(m.named_parameters(), grads):
        ref = T(g[f"inst.gsub.{k}"]).double()
        if gr is None:
            assert float(ref.abs().max()) == 0.0, k
            continue
        flat = gr.detach().contiguous().reshape(-1)
        rel_close(flat if flat.numel() <= 4096 else flat[::17], ref, 2e-3, atol=2e-3 * float(ref.abs().max()) * 0.05 + 1e-10, what=k)
        n += 1
    assert n >= 12
    seg = r.forward_segment_feature(m, rays, 0, False)
    rel_close(seg, g["seg"], 1e-3, what="seg")
    grads = torch.autograd.grad((seg * T(g["cot_seg"]).to(DEV)).sum(), list(m.parameters()), allow_unused=True)
    for (k, _), gr in zip(m.named_parameters(), grads):
        ref = T(g[f"seg.gsub.{k}"]).double()
        if gr is None:
            assert float(ref.abs().max()) == 0.0, k
            continue
        flat = gr.detach().contiguous().reshape(-1)
        rel_close(flat if flat.numel() <= 4096 else flat[::17], ref, 2e-3, atol=2e-3 * float(ref.abs().max()) * 0.05 + 1e-10, what=k)


def test_empty_and_ragged_chunks():
    """Rays that miss the box entirely (no in-box sample, no active sample) and a single-ray chunk."""
    cl, op, orender, ofld, olosses, orays = _import()
    res, C_, E = (9, 13, 17), 4, 3
    aabb = torch.tensor([[-0.3, -0.3, -0.3], [0.3, 0.3, 0.3]])
    P = op.add_blob(op.make_params(5, res, C_, E), res, 2.5, 0.45)
    m = build_model(cl, P, res, C_, E, -3.0)
    r = cl.TensoRFRenderer(aabb, list(res), semantic_weight_mode="softmax").to(DEV)
    cfg = orender.RenderCfg(aabb, res, density_shift=-3.0)
    miss = torch.tensor([[0.9, 0.9, -0.9, 0.0, 0.0, 1.0, 0.01, 1.2], [-0.8, 0.7, -0.9, 0.0, 0.0, 1.0, 0.01, 1.1]])
    for rays, white in ((miss, False), (miss, True), (miss[:1], True)):
        with torch.no_grad():
            o = orender.render_forward(P, rays, cfg, None, white)
            rgb, sem, inst, depth, _, dreg = r.forward(m, rays.to(DEV), 0, white, False)
        rel_close(rgb, o[0], 1e-3, atol=1e-6, what="rgb (miss)")
        rel_close(sem, o[1], 1e-3, atol=1e-5, what="sem (miss)")
        rel_close(inst, o[2], 1e-3, atol=1e-6, what="inst (miss)")
    hit = torch.tensor([[0.0, 0.0, -0.9, 0.0, 0.0, 1.0, 0.01, 1.9]])
    with torch.no_grad():
        o = orender.render_forward(P, hit, cfg, None, False)
        rgb, sem, inst, depth, _, dreg = r.forward(m, hit.to(DEV), 0, False, False)
    rel_close(rgb, o[0], 1e-3, what="rgb (single ray)")
    rel_close(sem, o[1], 1e-3, what="sem (single ray)")


# ============================================================================ losses (a16-a19), optimiser plumbing
def test_contrastive_golden_g8():
    cl, *_ = _import()
    g = load_golden("g8_losses")
    for tag in "abcd":
        f = T(g[f"con_{tag}.f"]).to(DEV).requires_grad_(True)
        L = cl.contrastive_loss(f, T(g[f"con_{tag}.y"]).to(DEV), 100.0)
        rel_close(L, g[f"con_{tag}.loss"], 1e-4, atol=1e-6, what=f"contrastive {tag}")
        gr = torch.autograd.grad(L, f)[0]
        rel_close(gr, g[f"con_{tag}.grad"], 1e-3, atol=1e-7, what=f"contrastive grad {tag}")


def test_slow_fast_golden_g8():
    cl, *_ = _import()
    g = load_golden("g8_losses")
    for tag in "abcd":
        f = T(g[f"sf_{tag}.feats"]).to(DEV).requires_grad_(True)
        L = cl.slow_fast_loss(f, T(g[f"sf_{tag}.y"]).to(DEV), T(g[f"sf_{tag}.conf"]).to(DEV))
        rel_close(L, g[f"sf_{tag}.loss"], 1e-4, atol=1e-6, what=f"slow_fast {tag}")
        gr = torch.autograd.grad(L, f)[0]
        rel_close(gr, g[f"sf_{tag}.grad"], 1e-3, atol=1e-7, what=f"slow_fast grad {tag}")


def test_slow_fast_large_vs_oracle():
    cl, op, orender, ofld, olosses, orays = _import()
    rng = np.random.default_rng(3)
    B, E = 1024, 3
    f = torch.from_numpy(rng.standard_normal((B, 2 * E)).astype(np.float32) * 0.5)
    y = torch.from_numpy(rng.zipf(1.6, size=B).clip(max=25).astype(np.int64))
    y[:B // 2][y[:B // 2] == 7] = 26          # a label present only in the fast half
    conf = torch.from_numpy(rng.uniform(0.1, 1, B).astype(np.float32))
    fo = f.clone().requires_grad_(True)
    Lo = olosses.slow_fast(fo, y, conf)
    go = torch.autograd.grad(Lo, fo)[0]
    fd = f.to(DEV).requires_grad_(True)
    L = cl.slow_fast_loss(fd, y.to(DEV), conf.to(DEV))
    rel_close(L, Lo.detach(), 1e-4, what="slow_fast 1024")
    rel_close(torch.autograd.grad(L, fd)[0], go, 1e-3, atol=1e-8, what="slow_fast 1024 grad")
    fo2 = f[:, :E].clone().requires_grad_(True)
    Lc = olosses.contrastive(fo2, y, 100.0)
    gc = torch.autograd.grad(Lc, fo2)[0]
    fd2 = f[:, :E].contiguous().to(DEV).requires_grad_(True)
    L2 = cl.contrastive_loss(fd2, y.to(DEV), 100.0)
    rel_close(L2, Lc.detach(), 1e-4, what="contrastive 1024")
    rel_close(torch.autograd.grad(L2, fd2)[0], gc, 1e-3, atol=1e-8, what="contrastive 1024 grad")


def test_tv_golden_g9_and_total():
    cl, op, *_ = _import()
    g = load_golden("g9_tv")
    res = tuple(int(x) for x in g["res"])
    P = op.make_params(int(g["seed"]), res, 2, 3)
    x = P["density_plane.1"].to(DEV).requires_grad_(True)
    L = cl.TVLoss()(x)
    rel_close(L, g["tv_plane1"], 1e-4, what="tv")
    rel_close(torch.autograd.grad(L, x)[0], g["tv_plane1_grad"], 1e-3, atol=1e-9, what="tv grad")
    m = build_model(cl, P, res, 2, 3, -10.0)
    m.zero_grad_arena()
    Lt = m.total_tv_loss(None, None, 1)
    rel_close(Lt, g["total_tv"], 1e-4, what="total tv")
    for k, gr in m.named_grad_views().items():
        key = f"tv.gsub.{k}"
        if key in g:
            flat = gr.contiguous(memory_format=torch.contiguous_format).reshape(-1) if gr.dim() == 4 else gr.contiguous().reshape(-1)
            rel_close(flat if flat.numel() <= 4096 else flat[::17], g[key], 1e-3, atol=1e-10, what=key)


def test_pixel_losses_adam_ema_vs_torch():
    from contrastive_lift_amd import _lib
    cl, op, orender, ofld, olosses, orays = _import()
    rng = np.random.default_rng(9)
    N, C_ = 777, 22
    rgb = torch.from_numpy(rng.uniform(0, 1, (N, 3)).astype(np.float32)).requires_grad_(True)
    gt = torch.from_numpy(rng.uniform(0, 1, (N, 3)).astype(np.float32))
    sem = torch.log(torch.softmax(torch.from_numpy(rng.standard_normal((N, C_)).astype(np.float32)), -1) + 1e-8).requires_grad_(True)
    probs = torch.softmax(torch.from_numpy(rng.standard_normal((N, C_)).astype(np.float32)), -1)
    conf = torch.from_numpy(rng.uniform(0, 1, N).astype(np.float32))
    cw = torch.ones(C_); cw[0] = 0.0
    mask = torch.from_numpy((rng.uniform(0, 1, N) > 0.2).astype(np.float32))
    l_rgb = torch.nn.functional.mse_loss(rgb * mask[:, None], gt * mask[:, None])
    l_sem = olosses.semantic_ce(sem, probs, conf * mask, cw)
    (1.0 * l_rgb + 0.1 * l_sem).backward()
    out2 = torch.zeros(2, device=DEV)
    g_rgb, g_sem = torch.empty((N, 3), device=DEV), torch.empty((N, C_), device=DEV)
    keep = [t.detach().to(DEV).contiguous() for t in (rgb, gt, sem, probs, conf, cw, mask)]   # keep alive across the launch
    _lib.call("clift_pixel_losses", *[_lib.ptr(t) for t in keep], N, C_, 1.0, 0.1, _lib.ptr(out2), _lib.ptr(g_rgb),
              _lib.ptr(g_sem), _lib.stream())
    rel_close(out2[0], l_rgb.detach(), 1e-4, what="mse")
    rel_close(out2[1], l_sem.detach(), 1e-4, what="ce")
    rel_close(g_rgb, rgb.grad, 1e-3, atol=1e-9, what="g_rgb")
    rel_close(g_sem, sem.grad, 1e-3, atol=1e-9, what="g_sem")
    # Adam: 3 steps against torch.optim.Adam with weight decay
    n = 10007
    p0 = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=1e-2, betas=(0.9, 0.99), weight_decay=1e-3)
    pd, md, vd = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for step in range(1, 4):
        gstep = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
        pt.grad = gstep.clone()
        opt.step()
        gdev = gstep.to(DEV)
        _lib.call("clift_adam", _lib.ptr(pd), _lib.ptr(gdev), _lib.ptr(md), _lib.ptr(vd), n, 1e-2, 0.9, 0.99, 1e-8, 1e-3, step, _lib.stream())
        torch.cuda.synchronize()
    rel_close(pd, pt.detach(), 1e-4, atol=1e-6, what="adam")
    s, f = torch.from_numpy(rng.standard_normal(n).astype(np.float32)), torch.from_numpy(rng.standard_normal(n).astype(np.float32))
    sd, fd = s.to(DEV), f.to(DEV)
    _lib.call("clift_ema", _lib.ptr(sd), _lib.ptr(fd), n, 0.9, _lib.stream())
    rel_close(sd, s * 0.9 + 0.1 * f, 1e-6, atol=1e-7, what="ema")


# ============================================================================ full-size, size-independent properties
def test_full_size_properties():
    """BASELINE config sizes (4096 rays, grid 128^3 => S = 440): identities that need no oracle run.
       (1) opacity + background transmittance == 1 per ray (telescoping product, eps 1e-10 per sample);
       (2) compositing is linear: instance map of (fast|slow) equals the two halves composited separately, and
           white-background rgb == black-background rgb + (1 - opacity) before the clamp;
       (3) the compacted sample list is strictly increasing and counts match n_active;
       (4) determinism of the forward (bit-identical on repeat)."""
    cl, op, orender, ofld, olosses, orays = _import()
    from contrastive_lift_amd import engine
    res, C_, E, N = (128, 128, 128), 22, 3, 4096
    aabb = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])
    P, rays, rng = scene(op, orays, 41, res, C_, E, N, img=64, amp=3.0, sg=0.35)
    m = build_model(cl, P, res, C_, E, -3.0)
    r = cl.TensoRFRenderer(aabb, list(res), semantic_weight_mode="softmax").to(DEV)
    assert r.n_samples == 440
    rays = rays.to(DEV)
    jit = torch.rand(N, device=DEV)
    with torch.no_grad():
        o1, c1 = engine.render_forward(m, r, rays, jit, False)
        o2, c2 = engine.render_forward(m, r, rays, jit, True)
        o3, c3 = engine.render_forward(m, r, rays, jit, False)
    rel_close(c1.ray_out[:, 0] + c1.ray_out[:, 2], torch.ones(N), 1e-5, atol=1e-5, what="opacity + bg == 1")
    assert torch.equal(o1["rgb"], o3["rgb"]) and torch.equal(o1["semantics"], o3["semantics"]) and torch.equal(o1["instances"], o3["instances"])
    rel_close(c2.rgb_raw, c1.rgb_raw + (1 - c1.ray_out[:, 0:1]), 1e-5, atol=1e-6, what="white bg linearity")
    idx = c1.act_idx[:c1.M]
    assert bool((idx[1:] > idx[:-1]).all())
    assert int(c1.ray_start[-1]) == c1.M and c1.M == int((c1.w > 1e-4).sum())
    frac_act = c1.M / (N * 440)
    assert 0.02 < frac_act < 0.6, frac_act
    # semantic map: exp(log-probs) sums to ~1 where the ray hit something
    hit = c1.ray_out[:, 0] > 0.5
    ps = torch.exp(o1["semantics"][hit]).sum(-1)
    rel_close(ps, torch.ones_like(ps), 1e-3, what="sum_c exp(sem) == 1")


# ============================================================================ training step (a20) vs the oracle's CPU trainer
def test_training_step_vs_oracle():
    """HotPathTrainer (engine-driven main pass + slow-fast instance pass, arena Adam) against oracle.train_step.CpuTrainer
    (torch autograd + torch.optim.Adam) on identical inputs, jitter and white-background draws: gradients of every
    parameter after the backward, then parameters after two optimizer steps."""
    cl, op, orender, ofld, olosses, orays = _import()
    from contrastive_lift_amd.trainer import HotPathTrainer, default_config
    from oracle.train_step import CpuTrainer
    res, C_, E, B, Bi = (24, 28, 32), 5, 3, 384, 160
    aabb = torch.tensor([[-0.9, -0.8, -0.7], [0.8, 0.9, 0.75]])
    P, rays, rng = scene(op, orays, 77, res, C_, E, B + Bi, amp=2.3, sg=0.42)
    rays_main, rays_inst = rays[:B].contiguous(), rays[B:].contiguous()
    rgbs = torch.from_numpy(rng.uniform(0, 1, (B, 3)).astype(np.float32))
    probs = torch.softmax(torch.from_numpy(rng.standard_normal((B, C_)).astype(np.float32)), -1)
    conf = torch.from_numpy(rng.uniform(0.2, 1, B).astype(np.float32))
    labels = torch.from_numpy(rng.integers(1, 6, Bi).astype(np.int64))
    iconf = torch.from_numpy(rng.uniform(0.2, 1, Bi).astype(np.float32))
    m = build_model(cl, P, res, C_, E, -3.0)
    r = cl.TensoRFRenderer(aabb, list(res), semantic_weight_mode="softmax").to(DEV)
    cfg = default_config(chunk=0, instance_optimization_epoch=0, late_semantic_optimization=0)
    tr = HotPathTrainer(m, r, cfg, current_epoch=4)
    ct = CpuTrainer(P, orender.RenderCfg(aabb, res, density_shift=-3.0), chunk=4096, epoch=4)
    for step in range(2):
        jit = torch.from_numpy(rng.uniform(0, 1, B).astype(np.float32))
        jit_i = torch.from_numpy(rng.uniform(0, 1, Bi).astype(np.float32))
        white = bool(step % 2)
        oc = ct.main_pass(rays_main, rgbs, probs, conf, jit, [white])
        oi = ct.instance_pass(rays_inst, labels, iconf, jit_i)
        batch0 = dict(rays=rays_main.to(DEV), rgbs=rgbs.to(DEV), probabilities=probs.to(DEV), confidences=conf.to(DEV), mask=None)
        tr.main_pass(batch0, jitter=jit.to(DEV), white_bg=white)
        rel_close(tr.last_outputs[0], oc["rgb"], 1e-3, what=f"step {step} rgb")
        rel_close(tr.last_outputs[1], oc["sem"], 1e-3, what=f"step {step} sem")
        rel_close(tr.losses[0], oc["loss_rgb"], 1e-3, what="loss_rgb")
        rel_close(tr.losses[1], oc["loss_sem"], 1e-3, what="loss_sem")
        rel_close(tr.losses[2], oc["loss_tv"], 1e-3, what="loss_tv")
        if step == 0:    # gradients (the arena keeps them after the optimizer step)
            gv = m.named_grad_views()
            for k, pref in ct.P.items():
                if k.startswith("render_instance_mlp"):
                    continue
                ref = pref.grad
                grad_close(gv[k].detach().cpu(), ref, what=f"main grad {k}")
        tr.instance_pass([dict(rays=rays_inst.to(DEV), instances=labels.to(DEV), confidences=iconf.to(DEV))], jitter=jit_i.to(DEV))
        rel_close(tr.losses[3], oi["loss"], 1e-3, what="slow-fast loss")
        if step == 0:
            gv = m.named_grad_views()
            for k, pref in ct.P.items():
                if k.startswith("render_instance_mlp.mlp."):
                    grad_close(gv[k].detach().cpu(), pref.grad, what=f"inst grad {k}")
    # parameters after two Adam steps of both optimizers + two EMA updates.  Adam's first steps move every weight by
    # ~lr regardless of gradient size, so the comparison is absolute in units of the learning rate.
    sd = m.state_dict()
    for k, pref in ct.P.items():
        lr = 1e-2 if k.split(".")[0].endswith(("_plane", "_line")) else 5e-4
        diff = float((sd[k].detach().cpu() - pref.detach()).abs().max())
        assert diff <= 0.1 * lr * 2 + 1e-7, f"param {k}: max |diff| {diff:.3e} vs lr {lr}"   # elements with |g| ~ eps amplify gradient round-off


def test_psnr_parity_over_a_training_trajectory():
    """north_star: "PSNR ... within 0.1".  Sixty full training steps (main pass + slow-fast instance pass, both Adam optimizers,
    EMA) from identical weights, batches, jitter and white-background draws: the HIP trainer's PSNR on the training rays stays
    within 0.1 dB of the CPU oracle's at every checkpoint of the trajectory, and the losses within 2 %."""
    cl, op, orender, ofld, olosses, orays = _import()
    from contrastive_lift_amd.trainer import HotPathTrainer, default_config
    from oracle.train_step import CpuTrainer
    res, C_, E, B, Bi, steps = (24, 28, 32), 5, 3, 512, 192, 60
    aabb = torch.tensor([[-0.9, -0.8, -0.7], [0.8, 0.9, 0.75]])
    P, rays, rng = scene(op, orays, 91, res, C_, E, B + Bi, amp=2.3, sg=0.42)
    rays_main, rays_inst = rays[:B].contiguous(), rays[B:].contiguous()
    # a learnable target: colours and labels that are smooth functions of the ray direction
    d = rays_main[:, 3:6]
    rgbs = (0.5 + 0.5 * torch.sin(3.0 * d + torch.tensor([0.0, 1.0, 2.0]))).contiguous()
    probs = torch.softmax(4.0 * torch.stack([torch.sin((k + 1.0) * d[:, k % 3]) for k in range(C_)], -1), -1).contiguous()
    conf = torch.from_numpy(rng.uniform(0.5, 1, B).astype(np.float32))
    labels = (1 + (rays_inst[:, 3] > 0).long() + 2 * (rays_inst[:, 4] > 0).long()).contiguous()
    iconf = torch.from_numpy(rng.uniform(0.5, 1, Bi).astype(np.float32))
    m = build_model(cl, P, res, C_, E, -3.0)
    r = cl.TensoRFRenderer(aabb, list(res), semantic_weight_mode="softmax").to(DEV)
    tr = HotPathTrainer(m, r, default_config(chunk=0, instance_optimization_epoch=0, late_semantic_optimization=0), current_epoch=4)
    ct = CpuTrainer(P, orender.RenderCfg(aabb, res, density_shift=-3.0), chunk=4096, epoch=4)
    batch0 = dict(rays=rays_main.to(DEV), rgbs=rgbs.to(DEV), probabilities=probs.to(DEV), confidences=conf.to(DEV), mask=None)
    ibatch = [dict(rays=rays_inst.to(DEV), instances=labels.to(DEV), confidences=iconf.to(DEV))]
    psnr = lambda a, b: float(-10.0 * torch.log10(((a - b) ** 2).mean()))
    worst = 0.0
    for step in range(steps):
        jit = torch.from_numpy(rng.uniform(0, 1, B).astype(np.float32))
        jit_i = torch.from_numpy(rng.uniform(0, 1, Bi).astype(np.float32))
        white = bool(step % 3 == 0)
        oc = ct.main_pass(rays_main, rgbs, probs, conf, jit, [white])
        oi = ct.instance_pass(rays_inst, labels, iconf, jit_i)
        tr.main_pass(batch0, jitter=jit.to(DEV), white_bg=white)
        tr.instance_pass(ibatch, jitter=jit_i.to(DEV))
        if step % 10 == 9 or step == steps - 1:
            p_cpu, p_gpu = psnr(oc["rgb"], rgbs), psnr(tr.last_outputs[0].cpu(), rgbs)
            worst = max(worst, abs(p_cpu - p_gpu))
            assert abs(p_cpu - p_gpu) < 0.1, (step, p_cpu, p_gpu)
            rel_close(tr.losses[1], oc["loss_sem"], 2e-2, what=f"step {step} loss_sem")
            rel_close(tr.losses[3], oi["loss"], 2e-2, atol=2e-3, what=f"step {step} slow-fast loss")
    assert p_cpu > psnr(torch.full_like(rgbs, 0.5), rgbs) + 1.0          # the trajectory actually learned something
    print(f"PSNR after {steps} steps: oracle {p_cpu:.3f} dB, HIP {p_gpu:.3f} dB; worst |delta| along the trajectory {worst:.4f} dB")


@pytest.mark.parametrize("fixture", ["g12_training_steps", "g12c_training_steps_contrastive", "g12s_training_steps_segments",
                                     "g12e_training_steps_sce", "g12l_training_steps_linear_assignment", "g12g_training_steps_grid_heads",
                                     "g12a_training_steps_argmax", "g12n_training_steps_nottaconf", "g12p_training_steps_noconf"])
def test_g12_reference_training_steps_on_gpu(fixture):
    replay_g12(fixture)


def test_g13_assign_clusters_vs_reference():
    """inference.assign_clusters (clift_nearest_centroid per thing class, disjoint label offsets, one-hot) reproduces the
    reference's RP:371-419 output exactly, including the case where a thing class never occurs."""
    from contrastive_lift_amd.inference import assign_clusters
    g = load_golden("g13_postprocess")
    cents = {2: g["cent2"], 3: g["cent3"]}
    n = int(g["n_img"])
    for feats, pre, want in ((g["all_thing"], "sem", g["onehot"]), (g["all_thing_b"], "semb", g["onehot_b"])):
        sems = [T(g[f"{pre}{j}"]) for j in range(n)]
        got = assign_clusters(feats, sems, cents, torch.device(DEV), num_images=n)
        assert tuple(got.shape) == tuple(want.shape)
        assert torch.equal(got.cpu().to(torch.float64), torch.from_numpy(want))


def _check_segment_tables(sc, g):
    """build_segment_tables against the reference's Segment*Dataset: segment count and order, per-segment ray sets / confidences."""
    items = sc.build_segment_tables()
    assert len(items) == int(g["seg.count"]) and [it["rays"].shape[0] for it in items] == list(g["seg.sizes"])
    for k in (0, len(items) - 1):
        rel_close(items[k]["rays"][:, 0:6], g[f"seg.{k}.rays"][:, 0:6], 1e-5, atol=1e-6, what="segment rays")
        rel_close(items[k]["confidences"], g[f"seg.{k}.conf"], 1e-6, what="segment confidences")
    b = sc.segment_batch(4, 10, 1)
    assert b["n_groups"] == 4 and b["rays"].shape[0] == b["group"].shape[0] == b["confidences"].shape[0] and int(b["group"].max()) == 3
    assert all(int((b["group"] == j).sum()) <= 10 for j in range(4))


def test_g14_mos_ray_tables_vs_reference_dataset(tmp_path):
    """MOSScene.rays_for (clift_gen_rays on the device, from the per-frame intrinsics and normalised camera matrix) against
    the ray table the REFERENCE's MOSDataset built for the same files (golden G14), native and resized image_dim; and the
    flat training tables / instance images built from them."""
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_synthetic_mos as gen
    from contrastive_lift_amd.data import MOSScene
    g = load_golden("g14_mos_dataset")
    root = gen.make_scene(str(tmp_path / "scene"), n_frames=int(g["n_frames"]), size=int(g["size"]), seed=int(g["seed"]),
                          invalid_frames=(int(g["invalid_frame"]),), trajectory_frames=4)
    for tag in ("native", "resized"):
        dim = tuple(int(x) for x in g[f"{tag}.dim"])
        sc = MOSScene(root, "train", dim, float(g["max_depth"]), device=DEV)
        traj = list(sc.trajectory_set("trajectory_blender"))          # predefined camera path (dataset/base.py:320-365)
        assert len(traj) == int(g[f"{tag}.traj.len"])
        for j in (0, 3):
            name, rays = traj[j]
            assert name == str(g[f"{tag}.traj.{j}.name"])
            ref = g[f"{tag}.traj.{j}.rays"]
            rel_close(rays[:, 0:6], ref[:, 0:6], 1e-5, atol=1e-6, what="trajectory rays")
            rel_close(rays[:, 6:8], ref[:, 6:8], 1e-4, what="trajectory near/far")
        for f in (int(x) for x in g["frames"]):
            rays = sc.rays_for(f)
            ref = g[f"{tag}.f{f}.rays"]
            rel_close(rays[:, 0:3], ref[:, 0:3], 1e-5, atol=1e-6, what="origins")
            rel_close(rays[:, 3:6], ref[:, 3:6], 1e-5, atol=1e-6, what="directions")
            rel_close(rays[:, 6:8], ref[:, 6:8], 1e-4, what="near/far")
        tabs = sc.build_train_tables()
        hw = dim[0] * dim[1]
        assert tabs["rays"].shape == (len(sc.train_indices) * hw, 8) and tabs["mask"].dtype == torch.bool
        j = sc.train_indices.index(5)
        rel_close(tabs["rays"][j * hw:(j + 1) * hw], g[f"{tag}.f5.rays"], 1e-4, atol=1e-6, what="table rays")
        assert torch.equal(tabs["mask"][:hw].cpu(), torch.from_numpy(g[f"{tag}.f0.mask"]))
        assert len(sc.instance_images) > 0 and all(int((im["instances"] == 0).sum()) == 0 for im in sc.instance_images)
    _check_segment_tables(MOSScene(root, "train", (32, 32), float(g["max_depth"]), device=DEV), g)


def test_g15_panopli_ray_tables_vs_reference_dataset(tmp_path):
    """PanopLiScene.rays_for (device ray generation) against the ray tables of the REFERENCE's PanopLiDataset (golden G15)."""
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_synthetic_panopli as gen
    from contrastive_lift_amd.data import PanopLiScene
    g = load_golden("g15_panopli_dataset")
    root = gen.make_scene(str(tmp_path / "scene"), n_frames=int(g["n_frames"]), size=int(g["size"]), seed=int(g["seed"]),
                          invalid_frames=(int(g["invalid_frame"]),))
    for tag in ("native", "resized"):
        dim = tuple(int(x) for x in g[f"{tag}.dim"])
        sc = PanopLiScene(root, "train", dim, float(g["max_depth"]), device=DEV)
        for f in (int(x) for x in g["frames"]):
            rays = sc.rays_for(f)
            ref = g[f"{tag}.f{f}.rays"]
            rel_close(rays[:, 0:3], ref[:, 0:3], 1e-5, atol=1e-6, what="origins")
            rel_close(rays[:, 3:6], ref[:, 3:6], 1e-5, atol=1e-6, what="directions")
            rel_close(rays[:, 6:8], ref[:, 6:8], 1e-4, what="near/far")
        tabs = sc.build_train_tables()
        assert tabs["probabilities"].shape[1] == int(g[f"{tag}.num_classes"]) and len(sc.instance_images) > 0
    _check_segment_tables(PanopLiScene(root, "train", (32, 32), float(g["max_depth"]), device=DEV), g)


# ============================================================================ field point API + grid surgery (8f rank 1)
def test_field_point_api_golden_g3():
    cl, op, *_ = _import()
    g = load_golden("g3_field")
    res = tuple(int(x) for x in g["res"])
    P = op.make_params(int(g["seed"]), res, int(g["C"]), int(g["E"]))
    m = build_model(cl, P, res, int(g["C"]), int(g["E"]), -10.0)
    xn, vd = T(g["xn"]).to(DEV), T(g["viewdirs"]).to(DEV)
    rel_close(m.compute_density_without_activation(xn), g["density_raw"], 1e-4, what="density_raw")
    rel_close(m.compute_density(xn), g["density"], 1e-3, what="density")
    feat = m.compute_appearance_feature(xn)
    rel_close(feat, g["app_feat"], 1e-3, what="app_feat")
    rel_close(m.render_appearance_mlp(vd, feat), g["rgb"], 1e-3, what="rgb")
    rel_close(m.render_semantic_mlp(None, m.compute_semantic_feature(xn)), g["sem"], 1e-3, what="sem")
    rel_close(m.render_instance_mlp(None, m.compute_instance_feature(xn)), g["inst"], 1e-3, what="inst")


def test_shrink_and_upsample_golden_g10():
    cl, op, *_ = _import()
    g = load_golden("g10_grid_ops")
    res = tuple(int(x) for x in g["res"])
    P = op.add_blob(op.make_params(int(g["seed"]), res, 2, 3), res, amplitude=2.5, sigma_g=0.3)
    m = build_model(cl, P, res, 2, 3, float(g["shift"]))
    r = cl.TensoRFRenderer(T(g["aabb"]), list(res), semantic_weight_mode="softmax").to(DEV)
    alpha, _ = r.get_dense_alpha(m)
    rel_close(alpha, g["dense_alpha"], 1e-3, atol=1e-6, what="dense alpha")
    assert r.update_bbox_aabb_and_shrink(m)
    rel_close(r.bbox_aabb, g["shrunk_aabb"], 1e-6, what="shrunk aabb")
    assert r.grid_dim.tolist() == [int(x) for x in g["shrunk_grid"]]
    assert r.n_samples == int(g["shrunk_n_samples"])
    rel_close(r.step_size, g["shrunk_step"], 1e-6, what="step after shrink")
    rel_close(m.density_plane[0], g["shrunk_density_plane0"], 1e-6, what="cropped density plane 0")
    rel_close(m.density_line[0], g["shrunk_density_line0"], 1e-6, what="cropped density line 0")
    rel_close(m.appearance_plane[2][:, ::7], g["shrunk_appearance_plane2"], 1e-6, what="cropped appearance plane 2")
    target = r.get_target_resolution(4000)
    assert list(target) == [int(x) for x in g["target_res"]]
    m.upsample_volume_grid(target)
    r.update_step_size(target)
    rel_close(m.density_plane[1], g["up_density_plane1"], 1e-4, atol=1e-6, what="upsampled density plane 1")
    rel_close(m.density_line[2], g["up_density_line2"], 1e-4, atol=1e-6, what="upsampled density line 2")
    assert r.n_samples == int(g["up_n_samples"])
    # the re-packed arena is live: a forward/backward still works and parameters are arena views
    assert m.get_parameter("density_plane.1").data_ptr() >= m.param_flat.data_ptr()
    rays = torch.tensor([[0.0, 0.0, -0.9, 0.0, 0.0, 1.0, 0.01, 1.9]], device=DEV)
    rgb, *_ = r.forward(m, rays, 0, False, False)
    assert bool(torch.isfinite(rgb).all())


def test_pq_scene_parity_after_training():
    """north_star: "PSNR/PQ_scene within 0.1".  The HIP trainer learns a scene whose labels are functions of the 3-D surface
    point (300 steps: main pass with one-hot semantic targets + slow-fast instance pass); the trained weights are then rendered
    on a held-out 40x40 view by the HIP renderer and by the CPU oracle, the instance embeddings of each render are clustered
    with the MeanShift pipeline (inference.cluster, same numpy seed) and scored with the panoptic-quality evaluator (pinned by
    goldens G11/G16) against the ground-truth panoptic map: PQ / SQ / RQ / mIoU (x100) and PSNR (dB) of the two renders of the
    same checkpoint agree to 0.1.  (Parity of the training trajectory itself is the previous tests' subject.)"""
    cl, op, orender, ofld, olosses, orays = _import()
    from contrastive_lift_amd.trainer import HotPathTrainer, default_config
    from contrastive_lift_amd.inference import render_rays, create_instances_from_semantics, cluster, ConfusionMatrix
    from contrastive_lift_amd.metrics import panoptic_quality
    res, C_, E, B, Bi, steps = (24, 28, 32), 5, 3, 640, 256, 300
    things, stuff = [3, 4], [0, 1, 2]
    aabb = torch.tensor([[-0.9, -0.8, -0.7], [0.8, 0.9, 0.75]])
    P = op.add_blob(op.make_params(123, res, C_, E), res, amplitude=2.3, sigma_g=0.42)
    rng = np.random.default_rng(124)
    cfg_o = orender.RenderCfg(aabb, res, density_shift=-3.0)

    def view_rays(eye, img):
        eye = np.asarray(eye, np.float64); f = -eye / np.linalg.norm(eye)
        rt = np.cross(f, [0.0, 1.0, 0.0]); rt /= np.linalg.norm(rt)
        M = np.eye(4); M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = rt, np.cross(f, rt), f, eye
        K = torch.tensor([[img * 0.8, 0, img / 2], [0, img * 0.8, img / 2], [0, 0, 1]])
        return orays.ray_table(img, img, K, torch.tensor(M, dtype=torch.float32)).contiguous()
    pool = torch.cat([view_rays(e, 48) for e in ((0.0, 0.1, -0.9), (0.35, -0.1, -0.8), (-0.35, 0.2, -0.78), (0.0, 0.45, -0.75))], 0)

    def ground_truth(rays):          # labels from the surface point of the INITIAL field (identical on both sides)
        with torch.no_grad():
            out, aux = orender.render_forward(P, rays, cfg_o, return_aux=True)
        p = rays[:, :3] + out[3][:, None] / aux["opacity"].clamp_min(1e-3)[:, None] * rays[:, 3:6]     # expected termination point
        sem = 1 + (p[:, 0] > 0).long() + 2 * (p[:, 1] > 0).long()              # classes 1..4 by quadrant; 3 and 4 are things
        inst = torch.where(sem >= 3, (sem - 3) * 2 + (p[:, 0].abs() > 0.1).long() + 1, torch.zeros_like(sem))   # two bands per thing class
        rgb = 0.5 + 0.5 * torch.sin(4.0 * p + torch.tensor([0.0, 1.0, 2.0]))
        return sem, inst, rgb.contiguous()
    sem_all, inst_all, rgb_all = ground_truth(pool)
    thing_idx = torch.nonzero(inst_all > 0)[:, 0]
    assert thing_idx.numel() > 4 * Bi // 2 and len(torch.unique(inst_all[thing_idx])) == 4
    m = build_model(cl, P, res, C_, E, -3.0)
    r = cl.TensoRFRenderer(aabb, list(res), semantic_weight_mode="softmax").to(DEV)
    tr = HotPathTrainer(m, r, default_config(chunk=0, instance_optimization_epoch=0, late_semantic_optimization=0), current_epoch=4)
    for step in range(steps):
        pick = torch.from_numpy(rng.choice(pool.shape[0], B, replace=False))
        ipick = thing_idx[torch.from_numpy(rng.choice(thing_idx.numel(), Bi, replace=False))]
        rays_main, rays_inst = pool[pick].contiguous(), pool[ipick].contiguous()
        rgbs = rgb_all[pick].contiguous()
        probs = (torch.nn.functional.one_hot(sem_all[pick], C_).float() * 0.9 + 0.02).contiguous()
        conf = torch.ones(B)
        labels, iconf = inst_all[ipick].contiguous(), torch.ones(Bi)
        jit = torch.from_numpy(rng.uniform(0, 1, B).astype(np.float32))
        jit_i = torch.from_numpy(rng.uniform(0, 1, Bi).astype(np.float32))
        tr.main_pass(dict(rays=rays_main.to(DEV), rgbs=rgbs.to(DEV), probabilities=probs.to(DEV), confidences=conf.to(DEV), mask=None),
                     jitter=jit.to(DEV), white_bg=True)
        tr.instance_pass([dict(rays=rays_inst.to(DEV), instances=labels.to(DEV), confidences=iconf.to(DEV))], jitter=jit_i.to(DEV))
    # held-out view
    view = view_rays((0.1, 0.05, -0.88), 40)
    gt_sem, gt_inst, gt_rgb = ground_truth(view)
    target = torch.stack([gt_sem, gt_inst], -1)
    with torch.no_grad():
        trained = {k: v.detach().cpu().clone() for k, v in m.state_dict().items() if k in P}
        o_rgb, o_sem, o_inst, *_ = orender.render_forward(trained, view, cfg_o, white_bg=True)
    g_rgb, g_sem, g_inst, _ = render_rays(m, r, view.to(DEV), 0, white_bg=True)

    def score(rgb, sem, inst):
        sem, inst = sem.detach().cpu(), inst.detach().cpu()
        feats = create_instances_from_semantics(inst[:, :E], sem, things)
        np.random.seed(7)
        onehot, _ = cluster(feats.numpy(), 0.15, "cpu", 1)
        ids = onehot[0].argmax(-1)
        pq, sq, rq = panoptic_quality(torch.stack([sem.argmax(-1), ids], -1), target, things, stuff)
        cm = ConfusionMatrix(C_, ignore_class=[])
        cm.add_batch(sem.argmax(-1).numpy(), gt_sem.numpy())
        ps = float(-10.0 * torch.log10(((rgb.detach().cpu() - gt_rgb) ** 2).mean()))
        return 100 * float(pq), 100 * float(sq), 100 * float(rq), 100 * float(cm.get_miou()), ps
    so, sg = score(o_rgb, o_sem, o_inst), score(g_rgb, g_sem, g_inst)
    print("PQ/SQ/RQ/mIoU/PSNR  oracle %s   HIP %s" % (["%.3f" % x for x in so], ["%.3f" % x for x in sg]))
    assert so[0] > 20.0, so                      # the scene was learned well enough for PQ to mean something
    for a, b, what in zip(so, sg, ("PQ", "SQ", "RQ", "mIoU", "PSNR")):
        assert abs(a - b) <= 0.1, (what, a, b)
