"""The split-bf16 encoder modes without a GPU: the switch accepts them, and the arithmetic they stand for (tests/ref_split_encoder.py)
is as much closer to the oracle's f32 encoder as the design claims."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def test_switch_accepts_split_modes(S):
    m = S.FPBasedResNetBottleneck()
    for mode in ('bf16x3', 'bf16x6', 'f32', 'bf16'):
        assert m.set_encoder_precision(mode) is m
        assert m.encoder_precision == mode
    with pytest.raises(ValueError):
        m.set_encoder_precision('fp8')
    assert m.encoder_precision == 'bf16'
    cfg = {'key': 'FPBasedResNetBottleneck', 'kwargs': {'num_bottleneck_channels': 24, 'num_target_channels': 256}}
    net = S.splittable_resnet(cfg, resnet_name='resnet50', skips_avgpool=False, skips_fc=False, num_classes=10)
    for mode in ('bf16x3', 'bf16x6'):
        net.set_encoder_precision(mode)
        assert net.bottleneck_layer.encoder_precision == mode
    with pytest.raises(ValueError):
        net.set_encoder_precision('fp8')
    assert net.bottleneck_layer.encoder_precision == 'bf16x6'


def test_restatement_orders_the_modes(R):
    """8 bench images: mismatch(bf16x6) <= mismatch(bf16x3) <= mismatch(bf16) / 100 against the oracle's f32 encoder."""
    import ref_split_encoder as rs
    from benchlib.model import shape_workload, synthetic_batch

    class Holder:
        pass
    torch.manual_seed(0)
    bl = R.FPBasedResNetBottleneck()
    holder = Holder()
    holder.bottleneck_layer = bl
    shape_workload(holder)
    bl.eval()
    x = synthetic_batch(8, torch.device('cpu'))
    eb = bl.entropy_bottleneck
    with torch.no_grad():
        ref_sym = eb.symbols(bl.encoder(x))
        rate = {ns: (eb.symbols(rs.split_encoder(bl, x, ns)) != ref_sym).float().mean().item() for ns in (1, 2, 3)}
    print('symbols', ref_sym.numel(), 'mismatch rates', rate)
    assert rate[1] > 0
    assert rate[3] <= rate[2] <= rate[1] / 100
