"""-m gpu: training path (HIP forward AND backward kernels under autograd: conv data / weight gradients on the
implicit-GEMM and wgrad kernels, the GDN1 backward kernels, with the entropy bottleneck's backward kernel in the same
graph) against the f32 CPU oracle's autograd.

Tolerance: activations, weights and gradients pass through bf16 operands with f32 accumulation on the device, so
parameter gradients are compared by relative L2 error per tensor (<= 6e-2) and the loss by 2e-2 relative.

This is NOT a test of the entropy-bottleneck backward kernel: it is f32 end to end, a wrong slot among its 59 sums or a
dropped factor passes at 6e-2, and every shape here (N * C < 1024, latents of at most 1024 pixels) launches it with one
plane per workgroup and one partial row per plane.  The kernel-level check -- float64 reference, f32-grade bound, every
launch shape -- is tests/test_gpu_eb_backward.py."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))


def _pair(S, R, dev):
    from recipe import build_oracle_bottleneck
    ref, x = build_oracle_bottleneck(R)
    m = S.FPBasedResNetBottleneck()
    m.load_state_dict({k: v.clone() for k, v in ref.state_dict().items()})
    return m.to(dev), ref, x


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def test_forward2train_gradients(S, R, dev):
    m, ref, x = _pair(S, R, dev)
    m.train()
    ref.train()
    torch.manual_seed(1)
    noise = torch.rand(2, 24, 7, 7) - 0.5
    target = torch.randn(2, 256, 8, 8)
    hooked = {}
    h = m.entropy_bottleneck.register_forward_hook(lambda mod, inp, out: hooked.update(out=out))

    def loss_fn(out, lik, tgt):
        return ((out - tgt) ** 2).sum() + 0.08 * (-lik.log2().sum())

    # oracle
    y_ref = ref.encoder(x)
    yh_ref, lik_ref = ref.entropy_bottleneck(y_ref, noise=noise)
    out_ref = ref.decoder(yh_ref)
    loss_ref = loss_fn(out_ref, lik_ref, target)
    loss_ref.backward()
    aux_ref = ref.aux_loss()
    aux_ref.backward()

    # device: drive the module exactly as a training box would (forward hook output feeds the rate term)
    from sc2bench_amd import autograd as A
    y = A.analysis_autograd(m, x.to(dev))
    y_hat, lik = m.entropy_bottleneck(y, noise=noise.to(dev))
    assert hooked['out'][0] is y_hat and hooked['out'][1] is lik
    out = A.synthesis_autograd(m, y_hat)
    loss = loss_fn(out, lik, target.to(dev))
    loss.backward()
    aux = m.aux_loss()
    aux.backward()
    h.remove()

    assert abs(loss.item() - loss_ref.item()) <= 2e-2 * abs(loss_ref.item())
    assert abs(aux.item() - aux_ref.item()) <= 1e-4 * abs(aux_ref.item())
    ref_grads = dict(ref.named_parameters())
    worst = {}
    for name, p in m.named_parameters():
        g_ref = ref_grads[name].grad
        assert p.grad is not None, name
        if g_ref is None or g_ref.norm() == 0:
            continue
        worst[name] = _rel(p.grad, g_ref)
    bad = {k: v for k, v in worst.items() if v > 6e-2}
    assert not bad, 'gradient mismatch: {}'.format(bad)
    assert torch.equal(m.entropy_bottleneck.quantiles.grad.cpu() != 0, ref.entropy_bottleneck.quantiles.grad != 0)


def test_module_forward_in_train_mode_and_updated_path(S, R, dev):
    m, ref, x = _pair(S, R, dev)
    m.train()
    out = m(x.to(dev))                      # not updated: noise path through the public forward
    assert out.requires_grad and out.shape == (2, 256, 8, 8)
    out.sum().backward()
    assert m.encoder[0].weight.grad is not None and m.decoder[4].weight.grad is not None
    assert m.entropy_bottleneck.matrices[0].grad is not None
    # after update(): encoder + bottleneck frozen by round + detach (layer.py:543-549)
    m.zero_grad()
    m.update()
    ref.update(force=True)
    ref.train()
    out2 = m(x.to(dev))
    out2_ref = ref(x)
    out2.sum().backward()
    out2_ref.sum().backward()
    assert m.encoder[0].weight.grad is None or float(m.encoder[0].weight.grad.abs().sum()) == 0.0
    assert _rel(m.decoder[4].weight.grad, ref.decoder[4].weight.grad) < 6e-2
    assert _rel(out2, out2_ref) < 0.1


def test_frozen_parameters_get_no_gradient(S, R, dev):
    m, _, x = _pair(S, R, dev)
    m.train()
    for p in m.encoder.parameters():
        p.requires_grad_(False)
    out = m(x.to(dev))
    out.sum().backward()
    assert all(p.grad is None for p in m.encoder.parameters())
    assert m.decoder[0].weight.grad is not None


STAGE1 = {   # the `train.stage1` block of the reference's Entropic-Student ResNet-50 config (beta = 0.08), as data
    'teacher': {'sequential': ['conv1', 'bn1', 'relu', 'maxpool', 'layer1', 'layer2', 'layer3', 'layer4'],
                'forward_hook': {'input': [], 'output': ['layer1', 'layer2', 'layer3', 'layer4']}, 'requires_grad': False},
    'student': {'sequential': ['bottleneck_layer', 'layer2', 'layer3', 'layer4'],
                'frozen_modules': ['layer2', 'layer3', 'layer4'],
                'forward_hook': {'input': [], 'output': ['bottleneck_layer', 'layer2', 'layer3', 'layer4',
                                                         'bottleneck_layer.entropy_bottleneck']}, 'requires_grad': True},
    'optimizer': {'key': 'Adam', 'kwargs': {'lr': 0.001}},
    'scheduler': {'key': 'MultiStepLR', 'kwargs': {'milestones': [5, 8], 'gamma': 0.1}},
    'criterion': {'key': 'WeightedSumLoss', 'kwargs': {'sub_terms': dict(
        [('layer{}'.format(i), {'criterion': {'key': 'MSELoss', 'kwargs': {'reduction': 'sum'}},
                                'criterion_wrapper': {'key': 'SimpleLossWrapper', 'kwargs': {
                                    'input': {'is_from_teacher': False, 'module_path': 'bottleneck_layer' if i == 1 else 'layer{}'.format(i), 'io': 'output'},
                                    'target': {'is_from_teacher': True, 'module_path': 'layer{}'.format(i), 'io': 'output'}}},
                                'weight': 1.0}) for i in (1, 2, 3, 4)] +
        [('bpp', {'criterion': {'key': 'BppLoss', 'kwargs': {'entropy_module_path': 'bottleneck_layer.entropy_bottleneck',
                                                             'reduction': 'sum'}}, 'weight': 0.08})])}},
}


def test_stage1_training_steps_reduce_the_loss(S, dev):
    """Entropic-Student stage 1 driven by the reference's config keys: teacher/student hooks, MSE-sum + 0.08 * bits,
    aux-loss backward, flat-bucket (single process) reducer, Adam.  A few steps on a fixed batch must lower the loss."""
    from sc2bench_amd import training as T
    from sc2bench_amd.resnet import resnet50
    torch.manual_seed(0)
    cfg = {'key': 'FPBasedResNetBottleneck', 'kwargs': {'num_bottleneck_channels': 24, 'num_target_channels': 256}}
    student = S.splittable_resnet(cfg, skips_avgpool=False, skips_fc=False).to(dev)
    teacher = resnet50().to(dev)
    stage = T.DistillationStage(teacher, student, STAGE1, dev)
    assert all(not p.requires_grad for p in student.layer3.parameters())
    assert stage.reducer.nbytes() == 4 * 1304168     # stage 1: exactly the bottleneck, one 5.2 MB bucket
    x = torch.rand(4, 3, 64, 64, device=dev)
    losses = []
    for _ in range(6):
        loss = stage.forward_process(x)
        losses.append(loss.item())
        assert torch.isfinite(loss)
        stage.post_forward_process(loss)
    stage.clean_modules()
    assert losses[-1] < losses[0], losses
    assert float(student.bottleneck_layer.encoder[0].weight.grad.abs().sum()) == 0.0   # zeroed after the step


def test_mse_term_on_the_bottleneck_output_inside_the_conv_backward(S, dev):
    """The layer-1 feature-matching MSE term sits on the decoder's last conv output: with `host_policy.mse_fused` it hands (its operands,
    scale) to that conv's autograd node, which adds 2 scale (y - t) to the incoming gradient in one pass (sc2_relu_bwd_mse_bf16, relu =
    0) -- the parameter gradients equal the gradient-tensor form's up to the roundings it saves."""
    from sc2bench_amd.frozen import mse_fast_path
    torch.manual_seed(5)
    x = torch.rand(4, 3, 64, 64, device=dev)
    grads = {}
    for fused in (True, False):
        torch.manual_seed(7)
        m = S.FPBasedResNetBottleneck().to(dev).train()
        m.output_format = 'bf16_nhwc'
        S.hip.configure(mse_fused=fused)
        try:
            torch.manual_seed(9)                      # the same noise draw in both runs
            out = m(x)
            assert out.dtype == torch.bfloat16 and (hasattr(out, '_sc2_mse_sink') or not fused)
            torch.manual_seed(13)
            t = (torch.randn(out.shape, device=dev) * 0.3).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            w = torch.randn(out.shape, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            loss = 0.41 * mse_fast_path(torch.nn.MSELoss(reduction='sum'), out, t) + (out.float() * w.float()).sum()
            loss.backward()
            grads[fused] = {n: p.grad.detach().float().clone() for n, p in m.named_parameters() if p.grad is not None}
        finally:
            S.hip.configure(mse_fused=True)
    assert grads[True].keys() == grads[False].keys() and len(grads[True]) >= 10
    for n in grads[True]:
        a, b = grads[True][n], grads[False][n]
        assert ((a - b).norm() / (b.norm() + 1e-12)).item() < 2e-2, n


@pytest.mark.parametrize('switch', ['train_fused_conv0', 'train_fused_conv2', 'train_fused_dec0'])
def test_fused_stages_in_the_training_forward(S, dev, switch):
    """`host_policy.train_fused_conv0` / `_conv2` / `_dec0`: encoder[0] + GDN1(96), encoder[2] + GDN1(48) resp. decoder[0] + IGDN1(512) of the training forward
    as the fused inference launch that also emits the conv output; the backward is the unfused one on that tensor.  Output and every
    parameter gradient agree with the unfused forward's up to the bf16 roundings the two forwards place differently."""
    torch.manual_seed(5)
    x = torch.rand(3, 3, 96, 80, device=dev)
    outs, grads = {}, {}
    for fused in (True, False):
        torch.manual_seed(7)
        m = S.FPBasedResNetBottleneck().to(dev).train()
        S.hip.configure(**{switch: fused})
        try:
            torch.manual_seed(9)
            out = m(x)
            torch.manual_seed(13)
            w = torch.randn(out.shape, device=dev)
            (out.float() * w).sum().backward()
            outs[fused] = out.detach().float().clone()
            grads[fused] = {n: p.grad.detach().float().clone() for n, p in m.named_parameters() if p.grad is not None}
        finally:
            S.hip.configure(**{switch: True})
    assert ((outs[True] - outs[False]).norm() / outs[False].norm()).item() < 1e-2
    assert grads[True].keys() == grads[False].keys() and len(grads[True]) >= 10
    for n in grads[True]:
        a, b = grads[True][n], grads[False][n]
        assert ((a - b).norm() / (b.norm() + 1e-12)).item() < 3e-2, n


@pytest.mark.parametrize('inplanes,planes,stride,hw,N', [(256, 128, 2, 28, 4), (512, 128, 1, 14, 6), (1024, 512, 2, 14, 8), (64, 16, 1, 10, 6)])
def test_trainable_bottleneck_block_on_the_bn_kernels(S, dev, inplanes, planes, stride, hw, N):
    """A torchvision-layout Bottleneck block in TRAINING mode under bf16 autocast (stage 2's student tail): `host_policy.bn_train_hip`
    sends its norm layers + ReLUs + residual add through sc2_bn_train_fwd / _bwd.  Both forms are compared with the SAME block run in
    f32: the HIP form (one bf16 rounding per norm layer) must be about as close to it as the torch / MIOpen bf16 modules (which
    round behind the norm, behind the add and behind the ReLU; within 2x: the exact check of the kernels is tests/test_gpu_kernels.py::
    test_bn_train_kernels) -- output, input gradient, every parameter gradient; the running
    statistics agree with the f32 run's."""
    import copy
    from sc2bench_amd.resnet import Bottleneck
    torch.manual_seed(inplanes + hw)
    ds = None
    if stride != 1 or inplanes != planes * 4:
        ds = torch.nn.Sequential(torch.nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False), torch.nn.BatchNorm2d(planes * 4))
    ref = Bottleneck(inplanes, planes, stride=stride, downsample=ds).to(dev).train()
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
    x0 = (torch.randn(N, inplanes, hw, hw, device=dev) + 0.2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = torch.randn(N, planes * 4, (hw - 1) // stride + 1, (hw - 1) // stride + 1, device=dev)
    res = {}
    for name, on in (('f32', False), ('torch', False), ('hip', True)):
        blk = copy.deepcopy(ref)
        S.hip.configure(bn_train_hip=on)
        try:
            x = (x0.float() if name == 'f32' else x0.clone()).requires_grad_(True)
            with torch.autocast(device_type='cuda', dtype=torch.bfloat16, enabled=name != 'f32'):
                y = blk(x)
            assert y.dtype == (torch.float32 if name == 'f32' else torch.bfloat16)
            (y.float() * w).sum().backward()
            res[name] = (y.detach().float(), x.grad.detach().float(), {n: p.grad.detach().float().clone() for n, p in blk.named_parameters()},
                         {n: b.detach().float().clone() for n, b in blk.named_buffers()})
        finally:
            S.hip.configure(bn_train_hip=True)

    def rel(a, b):
        return ((a - b).norm() / (b.norm() + 1e-12)).item()

    def closer(a_hip, a_torch, a_ref, what):
        eh, et = rel(a_hip, a_ref), rel(a_torch, a_ref)
        assert eh <= 2.0 * et + 5e-3, '{}: hip {:.4f} torch {:.4f} (relative to the f32 block)'.format(what, eh, et)
    closer(res['hip'][0], res['torch'][0], res['f32'][0], 'output')
    closer(res['hip'][1], res['torch'][1], res['f32'][1], 'input gradient')
    for n in res['f32'][2]:
        closer(res['hip'][2][n], res['torch'][2][n], res['f32'][2][n], n)
    for n in res['f32'][3]:
        assert rel(res['hip'][3][n], res['f32'][3][n]) < 1e-2, n
