"""CPU: which `train.perceptual_opt` loss terms the library runs (perceptual.check_perceptual_opt, called by PerceptualPlan before
anything is allocated): the Gram-matrix style term with criterion 'l1' is accepted, every other criterion is refused by name."""
import pytest

from satlas_super_resolution_amd.perceptual import check_perceptual_opt

BLOCK = {"type": "PerceptualLoss", "layer_weights": {"conv1_2": 0.1, "conv5_4": 1}, "vgg_type": "vgg19", "use_input_norm": True,
         "perceptual_weight": 1.0, "style_weight": 0, "range_norm": False, "criterion": "l1"}


@pytest.mark.parametrize("pw,sw", [(1.0, 0), (1.0, 1.0), (0.0, 1.0)])
def test_style_with_l1_is_accepted(pw, sw):
    check_perceptual_opt(dict(BLOCK, perceptual_weight=pw, style_weight=sw))


@pytest.mark.parametrize("criterion", ["l2", "fro", "ssim"])
@pytest.mark.parametrize("sw", [0, 1.0])
def test_other_criteria_are_refused_by_name(criterion, sw):
    with pytest.raises(NotImplementedError, match="criterion"):
        check_perceptual_opt(dict(BLOCK, criterion=criterion, style_weight=sw))


def test_other_extractors_are_refused():
    with pytest.raises(NotImplementedError, match="vgg_type"):
        check_perceptual_opt(dict(BLOCK, vgg_type="vgg16", style_weight=1.0))
