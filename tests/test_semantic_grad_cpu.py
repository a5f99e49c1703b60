"""CPU: the opt-in differentiable SemanticLoss has no CPU implementation and says so at construction."""
import pytest


def test_differentiable_semantic_loss_on_cpu_raises():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.losses import SemanticLoss
    with pytest.raises(M2TError, match="differentiable"):
        SemanticLoss(device="cpu", differentiable=True)
    sl = SemanticLoss(device="cpu")          # the default stays constructible (it raises on first use, as before)
    assert sl.differentiable is False
