"""Host side of multi-scale inference (no GPU): the size rule, the argument checks of driver.infer_label_maps_ms, and that the
default arguments of validation_iou / compute_sample_weights never reach the multi-scale path."""
import pytest
import torch


def test_scaled_size_rule():
    import driver
    assert driver.scaled_size(1024, 2048, 0.5) == (512, 1024)
    assert driver.scaled_size(1024, 2048, 0.75) == (768, 1536)
    assert driver.scaled_size(65, 81, 0.75) == (49, 61)              # 48.75 -> 49, 60.75 -> 61
    assert driver.scaled_size(65, 81, 0.5) == (33, 41)               # 32.5 -> 33 (half rounds up), 40.5 -> 41
    assert driver.scaled_size(65, 81, 1.0) == (65, 81)
    assert driver.scaled_size(33, 49, 1.25) == (41, 61)              # 41.25 -> 41, 61.25 -> 61
    assert driver.scaled_size(3, 5, 0.1) == (0, 1)                   # 0.3 -> 0: refused by infer_label_maps_ms
    for H, W, s in [(37, 53, 0.3), (1024, 2048, 1.75), (7, 9, 2.0)]:
        assert driver.scaled_size(H, W, s) == (int(H * s + 0.5), int(W * s + 0.5))


def test_infer_label_maps_ms_refuses_bad_scales_before_touching_the_network():
    import driver
    image = torch.zeros(1, 3, 3, 5)
    with pytest.raises(ValueError, match="no scale"):
        driver.infer_label_maps_ms(None, image, scales=())
    with pytest.raises(ValueError, match="10 sources"):
        driver.infer_label_maps_ms(None, image, scales=(0.5, 0.75, 1.0, 1.25, 1.5), flip=True)
    with pytest.raises(ValueError, match="9 sources"):
        driver.infer_label_maps_ms(None, image, scales=tuple(1.0 + 0.1 * i for i in range(9)), flip=False)
    with pytest.raises(ValueError, match="gives 0x1"):
        driver.infer_label_maps_ms(None, image, scales=(1.0, 0.1), flip=False)
    # eight sources are accepted by the check: 4 scales x 2 orientations, 8 scales unflipped
    assert len(driver._ms_plan(65, 81, (0.5, 0.75, 1.0, 1.25), True)) == 4
    assert len(driver._ms_plan(65, 81, tuple(1.0 + 0.1 * i for i in range(8)), False)) == 8
    # the pyramid launch is skipped only for scale 1.0 without flip
    assert driver._ms_plan(65, 81, (0.75, 1.0), False) == [(49, 61, True), (65, 81, False)]
    assert driver._ms_plan(65, 81, (0.75, 1.0), True) == [(49, 61, True), (65, 81, True)]


class _Stop(Exception):
    pass


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))

    def forward(self, image):
        raise _Stop("single-scale forward")


def test_default_arguments_take_the_single_scale_paths(monkeypatch):
    import driver

    def boom(*a, **k):
        raise AssertionError("the multi-scale path was taken")

    def single(*a, **k):
        raise _Stop("infer_label_maps")
    monkeypatch.setattr(driver, "infer_label_maps_ms", boom)
    monkeypatch.setattr(driver, "infer_label_maps", single)
    net, batch = _Net(), (torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(_Stop, match="single-scale forward"):
        driver.validation_iou(net, [batch])
    with pytest.raises(_Stop, match="infer_label_maps"):
        driver.compute_sample_weights(net, [(batch[0], [0])], 1)
    # and with scales or flip given, both do go through infer_label_maps_ms
    for kw in (dict(scales=(1.0,)), dict(flip=True)):
        with pytest.raises(AssertionError, match="multi-scale path"):
            driver.validation_iou(net, [batch], **kw)
        with pytest.raises(AssertionError, match="multi-scale path"):
            driver.compute_sample_weights(net, [(batch[0], [0])], 1, **kw)
