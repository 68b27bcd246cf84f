"""CPU side of the GemNet-OC "bf16_act" mode: the mode switch itself (no device work) and the C ABI surface of its entry points."""
import pytest


def test_set_gemm_precision_accepts_bf16_act_and_restores():
    from nabladft_amd import gemnet_oc
    assert gemnet_oc._PRECISION[0] == "f32"
    try:
        gemnet_oc.set_gemm_precision("bf16_act")
        assert gemnet_oc._PRECISION[0] == "bf16_act"
        assert gemnet_oc._use_bf16(256, 64) and gemnet_oc._use_bf16_act(256, 64, 512)          # behaves as "bf16" everywhere ...
        assert not gemnet_oc._use_bf16_act(255, 64) and not gemnet_oc._use_bf16_act(256, 64, 48)   # ... and keeps the shape rule for every product around a tensor
        assert not gemnet_oc.fused_pairs_available()
        gemnet_oc.set_gemm_precision("bf16")
        assert gemnet_oc._use_bf16(256, 64) and not gemnet_oc._use_bf16_act(256, 64)
        with pytest.raises(ValueError):
            gemnet_oc.set_gemm_precision("fp16")
        assert gemnet_oc._PRECISION[0] == "bf16"                                                 # a rejected name changes nothing
    finally:
        gemnet_oc.set_gemm_precision("f32")
    assert gemnet_oc._PRECISION[0] == "f32" and not gemnet_oc._use_bf16(4096, 512) and gemnet_oc.fused_pairs_available()


def test_new_entry_points_are_bound():
    from nabladft_amd.build import build
    build(verbose=False)
    from nabladft_amd import _lib
    lib = _lib.load()
    for name in ("nq_linear_forward_bf16_out", "nq_linear_weight_grad_bf16_x", "nq_gn_ssilu_backward_bf16"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.nq_abi_version() == 17                                # additions only
    assert lib.nq_linear_forward_bf16_out(None, 0, None, None, None, 0, None, 0.0, 0.0, 4, 4, 32, None) == 2      # NQ_ERR_ARG before any device work
