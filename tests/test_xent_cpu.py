"""ops.cross_entropy / ops.CrossEntropyLoss: argument errors and the module's repr (no GPU)."""
import pytest
import torch

from distributeddataparallel_amd.ops import CrossEntropyLoss
from distributeddataparallel_amd.ops.cross_entropy import cross_entropy


def _inputs():
    return torch.zeros(4, 10), torch.zeros(4, dtype=torch.long)


@pytest.mark.parametrize("eps", [-0.1, 1.0, 1.5, float("nan")])
def test_label_smoothing_outside_range_raises(eps):
    with pytest.raises(ValueError, match="label_smoothing"):
        cross_entropy(*_inputs(), label_smoothing=eps)
    with pytest.raises(ValueError, match="label_smoothing"):
        CrossEntropyLoss(label_smoothing=eps)


@pytest.mark.parametrize("z", [-1e-4, float("nan")])
def test_negative_z_loss_raises(z):
    with pytest.raises(ValueError, match="z_loss"):
        cross_entropy(*_inputs(), z_loss=z)
    with pytest.raises(ValueError, match="z_loss"):
        CrossEntropyLoss(z_loss=z)


def test_unknown_reduction_raises():
    with pytest.raises(ValueError, match="reduction"):
        cross_entropy(*_inputs(), reduction="batchmean")
    with pytest.raises(ValueError, match="reduction"):
        CrossEntropyLoss(reduction="batchmean")


def test_positional_signature_stays():
    x, t = _inputs()
    t[1] = 3
    assert torch.equal(cross_entropy(x, t, 3), torch.nn.functional.cross_entropy(x, t, ignore_index=3))
    with pytest.raises(TypeError):
        cross_entropy(x, t, 3, 0.1)  # the new arguments are keyword-only


def test_module_arguments_and_repr():
    m = CrossEntropyLoss()
    assert (m.ignore_index, m.label_smoothing, m.z_loss, m.reduction) == (-100, 0.0, 0.0, "mean")
    m = CrossEntropyLoss(ignore_index=3, label_smoothing=0.1, z_loss=1e-4, reduction="sum")
    assert repr(m) == "CrossEntropyLoss(ignore_index=3, label_smoothing=0.1, z_loss=0.0001, reduction='sum')"
    assert isinstance(m, torch.nn.Module) and not list(m.parameters())
    x, t = torch.randn(4, 10), torch.tensor([1, 3, 9, 0])
    assert torch.equal(m(x, t), cross_entropy(x, t, 3, label_smoothing=0.1, z_loss=1e-4, reduction="sum"))
