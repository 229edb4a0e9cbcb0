"""`sc2_seg_ce_forward` / `sc2_seg_ce_backward` (csrc/seg_loss.hip) on the device against tests/ref_seg_loss.py, the float64
restatement, under the tolerance rule derived in that file's docstring (checked on the CPU by tests/test_seg_loss_ref_cpu.py):
tol_p = 2^-24 (32 M + 4 C + 32) per pixel, tol_dx = g A 2^-24 (32 M + 4 C + 32 + K) per gradient element (+ 2^-8 |ref| for bf16).
Counts, reproducibility and the bytes around the gradient are exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ref_seg_loss as RL
from tests.test_gpu_seg_predict import LAYOUTS

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.bfloat16)
INDEXES = range(len(RL.CASES))


@pytest.fixture(autouse=True)
def _kernel_path(S):
    """every test here runs with `seg_loss_hip` on, whatever its default (bad targets must never reach torch's device assert)"""
    before = S.hip.host_policy.seg_loss_hip
    S.hip.configure(seg_loss_hip=True)
    yield
    S.hip.configure(seg_loss_hip=before)


def _name(dtype):
    return str(dtype).split('.')[1]


def dx_arena(layout, shape, dtype, dev):
    """-> (arena, view, owned): a NaN-filled flat buffer, a [N,C,h,w] view inside it in the layout under test, and the mask of the
    arena elements that belong to the view"""
    n, c, h, w = shape

    def carve(flat):
        if layout == 'nhwc':
            pitch = (c + 7) // 8 * 8
            return flat[64:64 + n * h * w * pitch].view(n, h, w, pitch)[..., :c].permute(0, 3, 1, 2)
        if layout == 'sliced':
            return flat[64:64 + n * (c + 2) * (h + 1) * (w + 3)].view(n, c + 2, h + 1, w + 3)[:, 1:c + 1, :h, 2:w + 2]
        return flat[64:64 + n * c * h * w].view(n, c, h, w)
    count = {'nhwc': n * h * w * ((c + 7) // 8 * 8), 'sliced': n * (c + 2) * (h + 1) * (w + 3), 'nchw': n * c * h * w}[layout] + 128
    arena = torch.full((count,), float('nan'), dtype=dtype, device=dev)
    owned = torch.zeros(count, dtype=torch.bool, device=dev)
    carve(owned).fill_(True)
    return arena, carve(arena), owned


def dx_tolerance(dx, tol, dtype):
    return tol + (2.0 ** -8 * np.abs(dx) if dtype == torch.bfloat16 else 0.0)


@pytest.mark.parametrize('index', INDEXES, ids=RL.CASE_IDS)
def test_forward_and_backward_every_layout_and_dtype(S, dev, index):
    n, c, (h, w), size, _, _ = RL.CASES[index]
    targets = RL.case_targets(index)
    assert {255, -1, c, c + 3, 0, c - 1} <= set(targets.flatten().tolist())
    t_dev = targets.to(dev)
    for dtype in DTYPES:
        x = RL.case_logits(index, _name(dtype))
        ref = RL.case_reference(index, _name(dtype))
        for layout, make in LAYOUTS.items():
            what = '{} {} {}'.format(RL.CASE_IDS[index], _name(dtype), layout)
            v = make(x, dev)
            res = S.hip.seg_ce_forward(v, size, t_dev, want_pixel_loss=True)
            counts = res.sums.view(torch.int64)[1:].tolist()
            assert counts == [ref.count, ref.n_bad], (what, counts)
            pixel = res.pixel_loss.cpu().numpy()
            assert not pixel[~ref.valid].any(), what
            RL.assert_close(pixel, ref.pixel_loss, ref.tol_p, what + ' pixel loss')
            RL.assert_close(res.lse, ref.lse, ref.tol_p, what + ' lse')
            mean = (res.sums[0] / res.sums.view(torch.int64)[1]).float()
            RL.assert_close(mean, ref.loss_mean, ref.tol_p, what + ' mean')
            RL.assert_close(res.sums[0].float(), ref.loss_sum, ref.count * ref.tol_p, what + ' sum')
            # without the optional outputs: the same sums, bit for bit
            lean = S.hip.seg_ce_forward(v, size, t_dev, want_lse=False)
            assert lean.lse is None and lean.pixel_loss is None and torch.equal(lean.sums.view(torch.int64), res.sums.view(torch.int64))
            for reduction, code, g_out in (('mean', S.hip.SEG_CE_MEAN, 1.0), ('sum', S.hip.SEG_CE_SUM, 0.75)):
                dx_ref, tol = ref.grad(reduction, g_out)
                arena, out, owned = dx_arena(layout, (n, c, h, w), dtype, dev)
                grad_out = torch.tensor(g_out, dtype=torch.float32, device=dev)
                got = S.hip.seg_ce_backward(v, size, t_dev, res.lse, res.sums, grad_out, reduction=code, out=out)
                assert got is out
                assert bool(torch.isnan(arena[~owned]).all()), what + ': written outside dx'
                assert not bool(torch.isnan(arena[owned]).any()), what + ': an element of dx was not written'
                RL.assert_close(out.float(), dx_ref, dx_tolerance(dx_ref, tol, dtype), '{} dx {}'.format(what, reduction))
            if c == 1:
                assert not out.float().any() and not pixel.any()
    # reduction 'none': a per-pixel factor (f32, NCHW)
    x = RL.case_logits(index, 'float32')
    ref = RL.case_reference(index, 'float32')
    gp = torch.rand(targets.shape, generator=torch.Generator().manual_seed(7)) - 0.3
    res = S.hip.seg_ce_forward(x.to(dev), size, t_dev)
    got = S.hip.seg_ce_backward(x.to(dev), size, t_dev, res.lse, res.sums, gp.to(dev), reduction=S.hip.SEG_CE_NONE)
    dx_ref, tol = ref.grad('none', gp.double().numpy())
    RL.assert_close(got, dx_ref, tol, RL.CASE_IDS[index] + ' dx none')


def test_two_launches_give_the_same_bits(S, dev):
    for index in (0, 6, 7):
        size = RL.CASES[index][3]
        t_dev = RL.case_targets(index).to(dev)
        for dtype in DTYPES:
            v = LAYOUTS['nhwc'](RL.case_logits(index, _name(dtype)), dev)
            runs = []
            for _ in range(2):
                res = S.hip.seg_ce_forward(v, size, t_dev)
                dx = S.hip.seg_ce_backward(v, size, t_dev, res.lse, res.sums, torch.ones((), device=dev))
                runs.append((res.sums.view(torch.int64).clone(), dx.contiguous().view(torch.int16 if dtype == torch.bfloat16 else torch.int32).clone()))
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), (index, dtype)


def test_all_ignored_gives_nan_loss_and_zero_gradient(S, dev):
    index = 0
    size = RL.CASES[index][3]
    x = RL.case_logits(index, 'float32').to(dev).requires_grad_(True)
    targets = torch.full_like(RL.case_targets(index), RL.IGNORE).to(dev)
    loss = S.dense.seg_cross_entropy(x, size, targets)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and bool(torch.isnan(loss))
    loss.backward()
    assert x.grad.shape == x.shape and not bool(x.grad.any())
    # one image of two ignored: that image's gradient is zero, the other's is not
    index = 2
    size = RL.CASES[index][3]
    t = RL.case_targets(index).clone()
    t[1] = RL.IGNORE
    x = RL.case_logits(index, 'float32').to(dev).requires_grad_(True)
    S.dense.seg_cross_entropy(x, size, t.to(dev)).backward()
    assert bool(x.grad[0].any()) and not bool(x.grad[1].any())


def test_strict_raises_on_a_bad_target(S, dev):
    index = 1
    size = RL.CASES[index][3]
    x = RL.case_logits(index, 'float32').to(dev)
    t = RL.case_targets(index)
    ref = RL.case_reference(index, 'float32')
    with pytest.raises(ValueError, match='{} targets'.format(ref.n_bad)):
        S.dense.seg_cross_entropy(x, size, t.to(dev), strict=True)
    clean = t.clone()
    clean[(clean < 0) | (clean >= x.shape[1])] = RL.IGNORE
    loss = S.dense.seg_cross_entropy(x, size, clean.to(dev), strict=True)
    RL.assert_close(loss, ref.loss_mean, ref.tol_p, 'strict, clean targets')      # bad targets are skipped: the same pixels count
    with pytest.raises(S.hip.Sc2Error):      # more than 64 classes: the kernel refuses, seg_cross_entropy takes torch
        S.hip.seg_ce_forward(torch.zeros(1, 65, 2, 2, device=dev), (4, 4), torch.zeros(1, 4, 4, dtype=torch.int64, device=dev))
    wide = torch.randn(1, 65, 2, 2, generator=torch.Generator().manual_seed(3)).to(dev)
    wide_t = torch.randint(0, 65, (1, 4, 4), generator=torch.Generator().manual_seed(4)).to(dev)
    want = F.cross_entropy(F.interpolate(wide, size=(4, 4), mode='bilinear', align_corners=False), wide_t, ignore_index=255)
    assert torch.equal(S.dense.seg_cross_entropy(wide, (4, 4), wide_t), want)


@pytest.mark.parametrize('reduction', ['mean', 'sum', 'none'])
def test_autograd_switch_on_against_switch_off(S, dev, reduction):
    """`seg_cross_entropy` through autograd on the kernels and on torch's device ops (the switch off): both within the rule of the
    float64 restatement"""
    for index in (0, 2, 7):
        size = RL.CASES[index][3]
        c = RL.CASES[index][1]
        ref = RL.case_reference(index, 'float32')
        clean = RL.case_targets(index).clone()
        clean[(clean < 0) | (clean >= c)] = RL.IGNORE      # torch asserts on them; the kernels skip them: the same valid pixels
        gp = torch.rand(clean.shape, generator=torch.Generator().manual_seed(7)) - 0.3
        results = {}
        default = S.hip.host_policy.seg_loss_hip
        for on in (True, False):
            S.hip.configure(seg_loss_hip=on)
            try:
                x = RL.case_logits(index, 'float32').to(dev).requires_grad_(True)
                loss = S.dense.seg_cross_entropy(x, size, clean.to(dev), reduction=reduction)
                assert loss.dtype == torch.float32
                if reduction == 'none':
                    loss.backward(gp.to(dev))
                else:
                    loss.backward()
            finally:
                S.hip.configure(seg_loss_hip=default)
            results[on] = (loss.detach(), x.grad)
        for on, (loss, grad) in results.items():
            what = '{} {} switch {}'.format(RL.CASE_IDS[index], reduction, 'on' if on else 'off')
            if reduction == 'none':
                RL.assert_close(loss, ref.pixel_loss, ref.tol_p, what + ' loss')
                dx_ref, tol = ref.grad('none', gp.double().numpy())
            else:
                want, scale = (ref.loss_mean, 1) if reduction == 'mean' else (ref.loss_sum, ref.count)
                RL.assert_close(loss, want, scale * ref.tol_p, what + ' loss')
                dx_ref, tol = ref.grad(reduction)
            RL.assert_close(grad, dx_ref, tol, what + ' dx')


def test_one_distillation_stage_step(S, dev):
    """The tiny segmentation model through `DistillationStage` with the inline PASCAL criterion, kernels against torch ops.
    Bounds.  Both paths see bit-identical logits (the forward is the same code), so per head each logits gradient lies within tol_dx of
    ONE float64 gradient, and the two are held to D = tol_dx of each other (the head's weight 1.0 / 0.5 is inside g); the losses to
    1.0 tol_p(out) + 0.5 tol_p(aux), the issue's 1.5 tol_p with each head's own M.  A 1x1 head's parameter gradients are sums of dx * feature (weight) and of dx (bias): they differ by at most
    sum D |feature| and sum D.  The backbone's gradient is linear in the gradient of the features, gf = W^T dx per pixel, which
    differs by at most Dg = |W|^T D; with J the float64 Jacobian of the features with respect to a backbone parameter the difference
    is at most sum |J| Dg.  On top of either, the f32 sums of torch's own backward: n u sum |terms|, n = the number of feature
    elements (more than the terms of any one sum), taken from the same |.| sums with the reference gradient in place of D."""
    from sc2bench_amd import training as T
    images, targets = RL.tiny_batch()
    grads, losses = {}, {}
    default = S.hip.host_policy.seg_loss_hip
    for on in (True, False):
        S.hip.configure(seg_loss_hip=on)
        try:
            model = RL.tiny_seg_model().to(dev)
            stage = T.DistillationStage(RL.tiny_seg_model(seed=9).to(dev), model, RL.pascal_stage_config(), dev)
            assert model.defer_resize is True
            loss = stage.forward_process(images.to(dev), targets.to(dev))
            losses[on] = loss.item()
            loss.backward()
            grads[on] = {k: p.grad.detach().double().cpu().numpy() for k, p in model.named_parameters()}
            stage.post_forward_process(stage.forward_process(images.to(dev), targets.to(dev)))      # and a whole step runs
            stage.clean_modules()
            assert model.defer_resize is False
        finally:
            S.hip.configure(seg_loss_hip=default)
    # float64 on the host: logits, their reference gradients and tolerances, features, the backbone Jacobian
    model = RL.tiny_seg_model().double()
    feats = model.backbone(images.double())
    heads = {'out': (model.classifier, 1.0), 'aux': (model.aux_classifier, 0.5)}
    size = tuple(images.shape[-2:])
    tol_loss, D, G = 0.0, {}, {}
    for key, (head, weight) in heads.items():
        ref = RL.Reference(head(feats[key]).detach(), size, targets.numpy())
        tol_loss += weight * ref.tol_p
        dx, tol = ref.grad('mean', weight)
        D[key], G[key] = np.broadcast_to(tol, dx.shape), np.abs(dx)
    print('stage loss: on {:.9f} off {:.9f}, tolerance {:.3e}'.format(losses[True], losses[False], tol_loss))
    assert abs(losses[True] - losses[False]) <= tol_loss
    n_terms = sum(f.numel() for f in feats.values())
    u = 2.0 ** -24
    names = {'out': 'classifier', 'aux': 'aux_classifier'}
    params = tuple(model.backbone.parameters())
    bound_backbone = [np.zeros(tuple(p.shape)) for p in params]
    for key, (head, _) in heads.items():
        f = np.abs(feats[key].detach().numpy())
        field = D[key] + n_terms * u * G[key]      # the two paths' difference, and the rounding of torch's own f32 sums
        RL.assert_close(grads[True][names[key] + '.weight'], grads[False][names[key] + '.weight'],
                        np.einsum('nchw,nkhw->ck', field, f)[:, :, None, None], 'stage {}.weight'.format(names[key]))
        RL.assert_close(grads[True][names[key] + '.bias'], grads[False][names[key] + '.bias'], field.sum((0, 2, 3)),
                        'stage {}.bias'.format(names[key]))
        dgf = np.einsum('ck,nchw->nkhw', np.abs(head.weight.detach().numpy()[:, :, 0, 0]), field)
        jac = torch.autograd.functional.jacobian(lambda *ps: _features_with(model.backbone, ps, images.double())[key], params, vectorize=True)
        for i, j in enumerate(jac):
            bound_backbone[i] += np.tensordot(dgf, np.abs(j.numpy()), axes=4)
    for (k, _), bound in zip(model.backbone.named_parameters(), bound_backbone):
        RL.assert_close(grads[True]['backbone.' + k], grads[False]['backbone.' + k], bound, 'stage backbone.' + k)


def _features_with(backbone, params, images):
    """the backbone's features as a function of its parameters (for the Jacobian)"""
    names = [k for k, _ in backbone.named_parameters()]
    return torch.func.functional_call(backbone, dict(zip(names, params)), (images,))
