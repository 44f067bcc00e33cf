"""The three adapter kernels that draw peft's per-module dropout masks themselves (RV_LORA_PEFT_MASKS on fused kernels):

    F   ops.lora_down_module_masks    t_g  = alpha dropout_g(x) A_g^T          (rv_gemm_nt_lora_masks_bf16)
    B1  ops.lora_dgrad_module_masks   dx   = R + sum_g mask_g o (dt_g A_g) / (1 - p)   (rv_gemm_nt_dropout_masks_bf16)
    B2  ops.lora_wgrad_module_masks   dA_g = dt_g^T dropout_g(x)               (rv_gemm_tn_lora_masks_bf16)

The reference of every case is CPU-side: masks from oracle.dropout_mask (pinned bit for bit to rv_dropout by
test_lora_gpu.py::test_dropout_mask_restatement_bit_exact), products in fp32 torch on bf16-rounded inputs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dropout_mask as DM  # noqa: E402

BF = torch.bfloat16
SEEDS = (1234567, 89, 2147480000)          # three distinct module seeds (the last one near the top of the 31-bit range)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _keep(rows, width, p, seed):
    """bool [rows, width]: rv_dropout(p, seed) keeps the element - the CPU restatement."""
    return torch.from_numpy(DM.keep_mask(rows * width, p, seed).reshape(rows, width))


def _ulp_of_larger(a, b):
    """One bf16 unit in the last place of max(|a|, |b|) (fp32 tensor; 8 significant bits)."""
    big = torch.maximum(a.float().abs(), b.float().abs())
    _, e = torch.frexp(big)                      # big = m 2^e, 0.5 <= m < 1
    return torch.ldexp(torch.ones_like(big), e - 8)


def _agreement(got, today, what, fails):
    """The criterion of test_lora_gpu.py::test_gemm_nn_lora_adapter_first_vs_adapter_last (fewer than 2 % of the elements differ)
    plus: none by more than one bf16 ulp of the larger value.  Prints the figures, records a miss."""
    diff = got != today
    frac = diff.float().mean().item()
    excess = ((got.float() - today.float()).abs() - _ulp_of_larger(got, today)).max().item() if diff.any() else 0.0
    n_over = int(((got.float() - today.float()).abs() > _ulp_of_larger(got, today)).sum()) if diff.any() else 0
    print(f"  {what}: {100 * frac:.4f} % of the elements differ from today's composition, {n_over} by more than one bf16 ulp")
    if not frac < 0.02:
        fails.append(f"{what}: {100 * frac:.3f} % of the elements differ (cap 2 %)")
    if n_over:
        fails.append(f"{what}: {n_over} elements differ by more than one bf16 ulp of the larger value (worst excess {excess:.3e})")


# ------------------------------------------------------------------------------------------------ 1. exact mask recovery
@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("K", [64, 256, 4096])
@pytest.mark.parametrize("M", [1, 127, 128, 4096 + 37])
def test_down_projection_recovers_every_modules_mask_exactly(M, K, G):
    """F with x = ones, p = 0.5 (keep factor exactly 2), alpha = 1 and A_g = the 64 one-hot rows that select column block b of x:
    t_g must be 2 * keep_g[:, 64 b : 64 b + 64] exactly, for every block b - pins the element indexing, the per-module keys and the
    tail rows."""
    from rlaif_v_amd import ops
    dev = _dev()
    p, seeds = 0.5, SEEDS[:G]
    want = torch.cat([2.0 * _keep(M, K, p, s).float() for s in seeds], dim=0).to(BF).to(dev)     # [G M, K]
    x = torch.ones(M, K, dtype=BF, device=dev)
    eye = torch.eye(64, dtype=BF, device=dev)
    for b in range(K // 64):
        A = torch.zeros(64 * G, K, dtype=BF, device=dev)
        for g in range(G):
            A[64 * g:64 * g + 64, 64 * b:64 * b + 64] = eye
        t = ops.lora_down_module_masks(x, A, p, seeds)
        for g in range(G):
            assert torch.equal(t[:, 64 * g:64 * g + 64], want[g * M:(g + 1) * M, 64 * b:64 * b + 64]), (b, g)


def test_down_projection_mask_ignores_the_leading_dimension():
    """lda > K: the mask index is row * K + col of the LOGICAL contiguous [M, K] input, whatever row stride is passed."""
    from rlaif_v_amd import ops
    dev = _dev()
    M, K, G, p = 300, 256, 3, 0.5
    xw = torch.ones(M, K + 64, dtype=BF, device=dev)
    xw[:, K:] = 7.0                                  # never read
    x = xw[:, :K]
    assert x.stride(0) == K + 64
    tw = torch.full((M, 64 * G + 8), -3.0, dtype=BF, device=dev)
    eye = torch.eye(64, dtype=BF, device=dev)
    for b in range(K // 64):
        A = torch.zeros(64 * G, K, dtype=BF, device=dev)
        for g in range(G):
            A[64 * g:64 * g + 64, 64 * b:64 * b + 64] = eye
        t = ops.lora_down_module_masks(x, A, p, SEEDS, out=tw[:, :64 * G])
        for g in range(G):
            want = (2.0 * _keep(M, K, p, SEEDS[g])[:, 64 * b:64 * b + 64].float()).to(BF).to(dev)
            assert torch.equal(t[:, 64 * g:64 * g + 64], want), (b, g)
    assert bool((tw[:, 64 * G:] == -3.0).all())      # nothing written beyond the G blocks


@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("M,N", [(1, 64), (127, 256), (4096 + 37, 4096), (300, 11008)])
def test_input_gradient_recovers_every_modules_mask_exactly(M, N, G):
    """B1 with dt_g = ones in its first column, row 0 of A_g = 2^g and R = 0 (p = 0.5): dx must be 2 * sum_g 2^g keep_g exactly."""
    from rlaif_v_amd import ops
    dev = _dev()
    p, seeds = 0.5, SEEDS[:G]
    dt = torch.zeros(M, 64 * G, dtype=BF, device=dev)
    aT = torch.zeros(N, 64 * G, dtype=BF, device=dev)
    want = torch.zeros(M, N)
    for g in range(G):
        dt[:, 64 * g] = 1.0
        aT[:, 64 * g] = 2.0 ** g
        want += 2.0 * 2.0 ** g * _keep(M, N, p, seeds[g]).float()
    want = want.to(BF).to(dev)
    zero = torch.zeros(M, N, dtype=BF, device=dev)
    assert torch.equal(ops.lora_dgrad_module_masks(dt, aT, p, seeds, residual=zero), want)
    assert torch.equal(ops.lora_dgrad_module_masks(dt, aT, p, seeds), want)                      # no residual at all
    assert torch.equal(ops.lora_dgrad_module_masks(dt, aT, p, seeds, out=zero, residual=zero), want)   # in place


@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("R,K", [(1, 64), (64, 256), (37, 4096), (4096 + 37, 4096), (2000, 11008)])
def test_weight_gradient_recovers_every_modules_mask_exactly(R, K, G):
    """B2 with x = ones (p = 0.5): dt_g one-hot in one row r0 -> row 0 of dA_g is 2 * keep_g[r0]; with at most 64 rows and
    dt_g[:, 0] = 1 -> row 0 of dA_g is 2 * the column sums of keep_g (<= 128: exact in bf16).  Every other row of dA is zero."""
    from rlaif_v_amd import ops
    dev = _dev()
    p, seeds = 0.5, SEEDS[:G]
    keeps = [_keep(R, K, p, s).float() for s in seeds]
    x = torch.ones(R, K, dtype=BF, device=dev)
    r0 = (R * 2) // 3
    dt = torch.zeros(R, 64 * G, dtype=BF, device=dev)
    for g in range(G):
        dt[r0, 64 * g] = 1.0
    dA = ops.lora_wgrad_module_masks(dt, x, p, seeds)
    for g in range(G):
        assert torch.equal(dA[64 * g], (2.0 * keeps[g][r0]).to(BF).to(dev)), g
        assert not bool(dA[64 * g + 1:64 * g + 64].any())
    if R <= 64:
        dt.zero_()
        for g in range(G):
            dt[:, 64 * g] = 1.0
        dA = ops.lora_wgrad_module_masks(dt, x, p, seeds)
        for g in range(G):
            assert torch.equal(dA[64 * g], (2.0 * keeps[g].sum(0)).to(BF).to(dev)), g
            assert not bool(dA[64 * g + 1:64 * g + 64].any())


# --------------------------------------------- 2. numerics, 3. agreement with today's composition, 4. bit stability
def _today_down(ops, x, A, p, seeds, alpha):
    t = torch.empty(x.shape[0], 64 * len(seeds), dtype=BF, device=x.device)
    for g, s in enumerate(seeds):
        ops.gemm_nt(ops.dropout(x, p, s), A[64 * g:64 * g + 64], out=t[:, 64 * g:64 * g + 64], alpha=alpha)
    return t


def _today_dgrad(ops, dt, aT, p, seeds, res):
    dx = res.clone()
    for g, s in enumerate(seeds):
        ops.gemm_nt_dropout(dt[:, 64 * g:64 * g + 64], aT[:, 64 * g:64 * g + 64], p, s, out=dx, residual=dx)
    return dx


def _today_wgrad(ops, dt, x, p, seeds):
    dA = torch.empty(64 * len(seeds), x.shape[1], dtype=BF, device=x.device)
    for g, s in enumerate(seeds):
        ops.gemm_tn_skinny(dt[:, 64 * g:64 * g + 64], ops.dropout(x, p, s), out=dA[64 * g:64 * g + 64])
    return dA


@pytest.mark.parametrize("p", [0.05, 0.25])
@pytest.mark.parametrize("M,K,G", [(29000, 4096, 1), (29000, 11008, 1), (29000, 4096, 2), (29000, 4096, 3), (1000, 256, 3)])
def test_numerics_agreement_and_bit_stability(M, K, G, p):
    """Random bf16 inputs at config 5's shapes (29,000 rows; widths 4096 and 11008) and a small odd one.  One set of inputs and one
    set of CPU masks (the mask of the [M, K] adapter input serves F, B2 and - same shape, same seeds - B1's [M, K] gradient):

    2. each kernel against the CPU product, by test_kernels_gpu.close as it stands (1.6e-2 of max |ref|, mean under half that);
    3. against today's composition (rv_dropout then rv_gemm_nt_bf16 / rv_gemm_nt_dropout_bf16 / rv_gemm_tn_bf16_splitk): B1 with
       G = 1 bit-identical; elsewhere fewer than 2 % of the elements differ and none by more than one bf16 ulp of the larger value.
       Expectation: F keeps the skinny kernel's K order (one 32x32x16 MFMA chain per 64-deep tile, tiles in order) -> 0 %; B1 adds
       each module's term with its own rounding to bf16 exactly like the G launches it replaces -> 0 % for every G; B2 runs gemm_tn_skinny's
       split plan for one module and sums the token rows like the shipped TN kernel (one 16x16x32 MFMA per 32-row tile, tiles in
       order, slabs in order) -> 0 %;
    4. a second run gives the same bits."""
    from rlaif_v_amd import ops
    from test_kernels_gpu import close
    dev = _dev()
    seeds, alpha = SEEDS[:G], 0.25
    g = torch.Generator(device=dev).manual_seed(M + K + G)
    x = torch.randn(M, K, device=dev, generator=g).to(BF)
    A = (torch.randn(64 * G, K, device=dev, generator=g) * 0.05).to(BF)          # stacked lora_A
    dt = (torch.randn(M, 64 * G, device=dev, generator=g) * 0.5).to(BF)
    res = torch.randn(M, K, device=dev, generator=g).to(BF)
    aT = A.t().contiguous()
    x_c, A_c, dt_c = x.cpu(), A.cpu().float(), dt.cpu().float()
    fails = []

    t = ops.lora_down_module_masks(x, A, p, seeds, alpha=alpha)
    dx = ops.lora_dgrad_module_masks(dt, aT, p, seeds, residual=res)
    dA = ops.lora_wgrad_module_masks(dt, x, p, seeds)
    # 4. bit stability (B1 also in place)
    assert torch.equal(ops.lora_down_module_masks(x, A, p, seeds, alpha=alpha), t)
    assert torch.equal(ops.lora_dgrad_module_masks(dt, aT, p, seeds, residual=res), dx)
    buf = res.clone()
    assert torch.equal(ops.lora_dgrad_module_masks(dt, aT, p, seeds, out=buf, residual=buf), dx)
    assert torch.equal(ops.lora_wgrad_module_masks(dt, x, p, seeds), dA)
    # 3. today's composition on the same inputs
    _agreement(t, _today_down(ops, x, A, p, seeds, alpha), "F", fails)
    today_dx = _today_dgrad(ops, dt, aT, p, seeds, res)
    if G == 1:
        assert torch.equal(dx, today_dx), "B1 with one module must be rv_gemm_nt_dropout_bf16 bit for bit"
    _agreement(dx, today_dx, "B1", fails)
    _agreement(dA, _today_wgrad(ops, dt, x, p, seeds), "B2", fails)
    # 2. the CPU products
    t_c, dA_c, dx_c = t.cpu(), dA.cpu(), dx.cpu()
    ref_dx = res.cpu().float()
    for gi, s in enumerate(seeds):
        mult = DM.multiplier(M, K, p, s)
        xd = (x_c.float() * mult).to(BF).float()                                   # the dropped operand as the MFMA sees it
        Ag, dtg = A_c[64 * gi:64 * gi + 64], dt_c[:, 64 * gi:64 * gi + 64]
        close(t_c[:, 64 * gi:64 * gi + 64], alpha * (xd @ Ag.t()), what=f"F module {gi}")
        close(dA_c[64 * gi:64 * gi + 64], dtg.t() @ xd, what=f"B2 module {gi}")
        del xd
        ref_dx += mult * (dtg @ Ag)
        del mult
    close(dx_c, ref_dx, what="B1")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("M,K,G", [(5000, 4096, 1), (5000, 4096, 3), (1000, 256, 2), (100, 64, 3)])
def test_p_zero_is_the_plain_gemm_bit_for_bit(M, K, G):
    """p = 0: F is rv_gemm_nt_bf16 (the streaming kernel from 4,096 rows, the 128x128 one below: same K order), B1 the chain of
    rv_gemm_nt_bf16 with dx as its own residual, B2 rv_gemm_tn_bf16_splitk with the same number of splits."""
    from rlaif_v_amd import ops
    dev = _dev()
    seeds = SEEDS[:G]
    g = torch.Generator(device=dev).manual_seed(M + K + G)
    x = torch.randn(M, K, device=dev, generator=g).to(BF)
    A = (torch.randn(64 * G, K, device=dev, generator=g) * 0.05).to(BF)
    dt = (torch.randn(M, 64 * G, device=dev, generator=g) * 0.5).to(BF)
    res = torch.randn(M, K, device=dev, generator=g).to(BF)
    aT = A.t().contiguous()
    assert torch.equal(ops.lora_down_module_masks(x, A, 0.0, seeds, alpha=0.25), ops.gemm_nt(x, A, alpha=0.25))
    dx = res.clone()
    for gi in range(G):
        ops.gemm_nt(dt[:, 64 * gi:64 * gi + 64], aT[:, 64 * gi:64 * gi + 64], out=dx, residual=dx)
    assert torch.equal(ops.lora_dgrad_module_masks(dt, aT, 0.0, seeds, residual=res), dx)
    assert torch.equal(ops.lora_wgrad_module_masks(dt, x, 0.0, seeds, splits=6), ops.gemm_tn_skinny(dt, x, splits=6))


def test_wrappers_refuse_bad_shapes():
    from rlaif_v_amd import ops
    dev = _dev()
    x = torch.ones(8, 96, dtype=BF, device=dev)
    with pytest.raises(RuntimeError, match="rv_gemm_nt_lora_masks_bf16"):
        ops.lora_down_module_masks(x, torch.ones(64, 96, dtype=BF, device=dev), 0.1, [1])
    with pytest.raises(ValueError, match="module seeds"):
        ops.lora_down_module_masks(x, torch.ones(256, 96, dtype=BF, device=dev), 0.1, [1, 2, 3, 4])
    with pytest.raises(ValueError, match="must be"):
        ops.lora_down_module_masks(x, torch.ones(64, 96, dtype=BF, device=dev), 0.1, [1, 2])
    with pytest.raises(RuntimeError, match="rv_gemm_tn_lora_masks_bf16"):
        ops.lora_wgrad_module_masks(torch.ones(8, 64, dtype=BF, device=dev), x, 1.0, [1])
    with pytest.raises(RuntimeError, match="rv_gemm_nt_dropout_masks_bf16"):
        ops.lora_dgrad_module_masks(torch.ones(8, 64, dtype=BF, device=dev), torch.ones(96, 64, dtype=BF, device=dev), 0.1, [1])
    assert not ops.lora_module_masks_ok(96, 64) and not ops.lora_module_masks_ok(128, 128) and ops.lora_module_masks_ok(11008, 64)
