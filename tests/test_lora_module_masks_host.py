"""CPU tests of the three per-module-mask adapter entry points (RV_LORA_PEFT_MASKS on fused kernels): declared in the header,
exported by the library, additive in ABI 7, and every bad shape is refused through the ABI before anything is launched (no GPU
exists here, so a launch would be an error of its own)."""
import pytest

NAMES = ("rv_gemm_nt_lora_masks_bf16", "rv_gemm_nt_dropout_masks_bf16", "rv_gemm_tn_lora_masks_bf16")


def _lib():
    import __graft_entry__ as g
    g.build()
    from rlaif_v_amd import hip
    return hip.lib()


def _call(lib, name, rows=128, K=256, G=2, p=0.25):
    """The entry point with null operands: only the argument checks can answer."""
    if name == "rv_gemm_nt_lora_masks_bf16":          # X, ldx, A, lda, T, ldt, M, K, G, alpha, p, seeds, stream
        return lib.lib.rv_gemm_nt_lora_masks_bf16(None, K, None, K, None, 64 * G, rows, K, G, 1.0, p, 1, 2, 3, None)
    if name == "rv_gemm_nt_dropout_masks_bf16":       # dT, lddt, AT, ldat, C, ldc, M, N, G, residual, ldr, p, seeds, stream
        return lib.lib.rv_gemm_nt_dropout_masks_bf16(None, 64 * G, None, 64 * G, None, K, rows, K, G, None, 0, p, 1, 2, 3, None)
    return lib.lib.rv_gemm_tn_lora_masks_bf16(None, 64 * G, None, K, None, K, rows, K, G, p, 1, 2, 3, 4, None, None)


def test_entry_points_declared_and_exported_in_abi_7():
    lib = _lib()
    for name in NAMES:
        assert name in lib.decls, name
        assert hasattr(lib.lib, name), name
    assert lib.lib.rv_abi_version() == 7
    # the seeds travel as three ints, the last argument is the stream
    for name in NAMES:
        args = [a for _, a in lib.decls[name][1]]
        assert args[-1] == "stream" and {"seed0", "seed1", "seed2", "G", "p"} <= set(args), (name, args)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("bad", [dict(K=96), dict(G=4), dict(G=0), dict(p=1.0), dict(p=-0.5)])
def test_bad_shapes_are_refused_without_a_launch(name, bad):
    lib = _lib()
    assert _call(lib, name, **bad) == 1, (name, bad)
    assert name in lib.last_error(), (name, bad, lib.last_error())


@pytest.mark.parametrize("name", NAMES)
def test_null_operands_are_refused(name):
    """A well-shaped call with null pointers is an argument error too, not a launch."""
    lib = _lib()
    assert _call(lib, name) == 1
    assert name in lib.last_error()
