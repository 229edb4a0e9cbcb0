"""GPU: the detection training kernels (csrc/detect.hip: sc2_box_match, sc2_roi_align_backward) against tests/ref_det_train.py, the
RPN and the RoI heads in training mode on them against the same modules on torch ops, and one Faster R-CNN training step."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_detection as RD  # noqa: E402
import ref_det_train as RT  # noqa: E402

pytestmark = pytest.mark.gpu

I32_SENTINEL = 0x5A5A5A5A
SETTINGS = [(low, high, allow) for low, high in ((0.3, 0.7), (0.5, 0.5)) for allow in (False, True)]


# ------------------------------------------------------------------------------------------------------------ matcher
def _match_run(S, dev, gts, cands, low, high, allow):
    """one call over the images -> nothing; asserts matches and best_iou equal the reference bit for bit, inside sentinel arenas"""
    want_m, want_b = RT.match_ref_batch(gts, cands, low, high, allow)
    total = sum(c.shape[0] for c in cands)
    arena_m = torch.full((total + 512,), I32_SENTINEL, dtype=torch.int32, device=dev)
    arena_b = torch.full((total + 512,), float('nan'), dtype=torch.float32, device=dev)
    gt = torch.from_numpy(np.concatenate(gts).astype(np.float32).reshape(-1, 4)).to(dev)
    cand = torch.from_numpy(np.concatenate(cands).astype(np.float32)).to(dev)
    m, b = S.hip.box_match(gt, [g.shape[0] for g in gts], cand, [c.shape[0] for c in cands], low, high, allow,
                           out=(arena_m[256:256 + total], arena_b[256:256 + total]))
    torch.cuda.synchronize()
    assert m.data_ptr() == arena_m[256:].data_ptr()
    hm, hb = arena_m.cpu().numpy(), arena_b.cpu().numpy()
    assert np.all(hm[:256] == I32_SENTINEL) and np.all(hm[256 + total:] == I32_SENTINEL), 'box_match wrote outside matches'
    assert np.all(np.isnan(hb[:256])) and np.all(np.isnan(hb[256 + total:])), 'box_match wrote outside best_iou'
    assert not np.any(hm[256:256 + total] == I32_SENTINEL) and not np.any(np.isnan(hb[256:256 + total])), 'an element was left unwritten'
    assert np.array_equal(hm[256:256 + total], want_m), (low, high, allow)
    assert np.array_equal(hb[256:256 + total].view(np.uint32), want_b.view(np.uint32)), (low, high, allow)
    # without best_iou
    only, none = S.hip.box_match(gt, [g.shape[0] for g in gts], cand, [c.shape[0] for c in cands], low, high, allow, want_iou=False)
    assert none is None and np.array_equal(only.cpu().numpy(), want_m)


# one size past every cap of the two launches: a workgroup of the second launch covers MATCH_CAND_PER_WG = 1024 candidates, one of the
# first MATCH_CHUNK = 2048 (4097 = two chunks and one candidate: three workspace rows, five workgroups of the second launch); the
# kernels stage MATCH_GT_TILE = 64 gt boxes at a time (65: a second tile of one box).  The grid itself has no cap below 2^31 / 1024.
@pytest.mark.parametrize('G', [0, 1, 3, 37, 65])
@pytest.mark.parametrize('A', [1, 63, 64, 65, 1000, 4097])
def test_box_match_equals_sequential_reference(S, dev, A, G):
    assert (S.hip.MATCH_CAND_PER_WG, S.hip.MATCH_CHUNK, S.hip.MATCH_GT_TILE) == (1024, 2048, 64)
    gt, cand = RT.match_boxes_case(A, G, seed=A * 3 + G)
    for low, high, allow in SETTINGS:
        _match_run(S, dev, [gt], [cand], low, high, allow)


def test_box_match_three_images(S, dev):
    """G = (0, 5, 2) with unequal A: offsets into both arrays, an image without gt boxes in front"""
    gts, cands = [], []
    for i, (A, G) in enumerate(((700, 0), (2500, 5), (130, 2))):
        gt, cand = RT.match_boxes_case(A, G, seed=50 + i)
        gts.append(gt)
        cands.append(cand)
    for low, high, allow in SETTINGS:
        _match_run(S, dev, gts, cands, low, high, allow)


def test_box_match_quarter_grid(S, dev):
    """coordinates on the quarter-pixel grid: exact ties and exact threshold hits (tests/test_det_train_ref_cpu.py asserts this very
    case holds at least one tie, one restored low-quality match and maxima of exactly 0.5 and 0.7)"""
    gt, cand = RD.quarter_grid_boxes(12, seed=12)[0], RD.quarter_grid_boxes(500, seed=500)[0]
    on, best, restored, tied = RT.match_ref(gt, cand, 0.5, 0.7, True)
    assert tied.sum() >= 1 and (on != RT.match_ref(gt, cand, 0.5, 0.7, False)[0]).sum() >= 1
    for low, high, allow in SETTINGS + [(0.5, 0.7, False), (0.5, 0.7, True)]:
        _match_run(S, dev, [gt], [cand], low, high, allow)
    _match_run(S, dev, [np.array([[5, 5, 5, 5], [0, 0, 2, 2]], dtype=np.float32)] * 2, [np.array([[5, 5, 5, 5], [0, 0, 2, 2]], dtype=np.float32),
                                                                                        np.array([[5, 5, 5, 5]], dtype=np.float32)], 0.3, 0.7, True)


def test_box_match_refuses_malformed_offsets(S, dev):
    gt, cand = RT.match_boxes_case(100, 4, seed=9)
    tg, tc = torch.from_numpy(gt).to(dev), torch.from_numpy(cand).to(dev)
    m = torch.full((100,), I32_SENTINEL, dtype=torch.int32, device=dev)
    b = torch.full((100,), float('nan'), dtype=torch.float32, device=dev)
    bad = [([0, 3, 2, 4], [0, 30, 60, 100]),        # gt offsets decrease
           ([0, 2, 4], [0, 60, 50]),                # candidate offsets decrease
           ([0, 2, 5], [0, 50, 100]),               # past the gt rows
           ([0, 2, 4], [0, 50, 101]),               # past the candidate rows
           ([1, 2, 4], [0, 50, 100]),               # does not start at 0
           ([0, 2, 4], [0, 50, 99])]                # does not cover the candidates
    for g_off, a_off in bad:
        with pytest.raises(ValueError, match='offsets'):
            S.hip.box_match_offsets(tg, g_off, tc, a_off, 0.3, 0.7, True, out=(m, b))
    with pytest.raises(ValueError, match='NaN'):
        S.hip.box_match_offsets(tg, [0, 4], tc, [0, 100], float('nan'), 0.7, True, out=(m, b))
    torch.cuda.synchronize()
    assert torch.all(m == I32_SENTINEL) and torch.all(torch.isnan(b)), 'a refused call launched something'
    S.hip.box_match_offsets(tg, [0, 2, 4], tc, [0, 50, 100], 0.3, 0.7, True, out=(m, b))       # the well-formed call writes everything
    assert not torch.any(m == I32_SENTINEL) and not torch.any(torch.isnan(b))


# ------------------------------------------------------------------------------------------------------------ RoIAlign backward
_REF_CACHE = {}


def _backward_case(C, P, K, seed, mode, rois_levels=None):
    """(grad_out, rois, levels, reference) of one case, computed once"""
    key = (C, P, K, seed, mode)
    if key not in _REF_CACHE:
        if rois_levels is None:
            rois, levels, dropped = RD.roi_cases(K, seed, P, 2, mode)
            assert dropped <= 0.05 * K, '{} of {} RoIs fell into the exclusion band: pick another seed'.format(dropped, K)
        else:
            rois, levels = rois_levels
        g = np.random.RandomState(seed + 100).randn(len(rois), C, P, P).astype(np.float32)
        _REF_CACHE[key] = (g, rois, levels, RT.roi_align_backward_ref(g, RD.MAPS, RD.SCALES, rois, levels, 2, P, 2))
    return _REF_CACHE[key]


def _backward_run(S, dev, C, P, case, name):
    g, rois, levels, (want, cnt, mag) = case
    K = len(rois)
    arenas, outs = [], []
    for h, w in RD.MAPS:
        total = 2 * h * w * C
        arena = torch.full((total + 2048,), float('nan'), dtype=torch.float32, device=dev)
        arenas.append(arena)
        outs.append(arena[1024:1024 + total].view(2, h, w, C))
    tg = torch.from_numpy(g).to(dev).reshape(K, C, P, P)
    tr = torch.from_numpy(np.asarray(rois, dtype=np.float32).reshape(K, 5)).to(dev)
    tl = torch.from_numpy(np.asarray(levels)).to(torch.int32).to(dev)
    got = S.hip.roi_align_backward(tg, RD.MAPS, RD.SCALES, tr, tl, 2, 2, out=outs)
    torch.cuda.synchronize()
    worst = 0.0
    for l, (arena, (h, w)) in enumerate(zip(arenas, RD.MAPS)):
        total = 2 * h * w * C
        host = arena.cpu().numpy()
        assert np.all(np.isnan(host[:1024])) and np.all(np.isnan(host[1024 + total:])), 'roi_align_backward wrote outside map {}'.format(l)
        inside = host[1024:1024 + total]
        assert not np.any(np.isnan(inside)), 'roi_align_backward left an element of map {} unwritten'.format(l)
        err = np.abs(inside.reshape(2, h, w, C).transpose(0, 3, 1, 2).astype(np.float64) - want[l])
        bound = RT.roi_backward_bound(cnt, mag)[l]
        assert np.all(err[bound == 0] == 0), 'map {}: a gradient where no sample lands'.format(l)
        if np.any(bound > 0):
            worst = max(worst, (err[bound > 0] / bound[bound > 0]).max())
    print('roi_align_backward {} C={} P={} K={}: max |err| / bound = {:.4f}'.format(name, C, P, K, worst))
    assert worst <= 1.0
    again = S.hip.roi_align_backward(tg, RD.MAPS, RD.SCALES, tr, tl, 2, 2)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), 'two calls on the same inputs differ'
    return (tg, tr, tl), got


@pytest.mark.parametrize('K,seed', [(1, 11), (37, 12), (300, 13)])
@pytest.mark.parametrize('P', [7, 2])
@pytest.mark.parametrize('C', [8, 256])
def test_roi_align_backward_equals_reference(S, dev, C, P, K, seed):
    """per map element |err| <= (2^-13 + n * 2^-24) * A against the float64 adjoint on the same f32 inputs, n the number of samples
    that touch the element (within 1 + 2^-10 px per axis) and A the sum of |g| / S^2 over them: an f32 sample lies within 2^-15.4 px of
    the float64 one and each axis weight has slope 1, so a product of two weights moves by at most 2^-14.4 -- 2^-13 leaves a factor
    2.6; the second term is the f32 summation.  Every element is written (zeros where nothing lands), none outside; two calls give the
    same bits.
    Observed on an MI355X, maximum over these cases and the four tests below: 0.028 of the bound (C = 256, P = 2, K = 300); 300 copies of one
    RoI: 0.0003."""
    _backward_run(S, dev, C, P, _backward_case(C, P, K, seed, 'mixed'), 'mixed')


@pytest.mark.parametrize('mode', ['one', 'skip'])
def test_roi_align_backward_one_level_and_an_unused_level(S, dev, mode):
    _backward_run(S, dev, 256, 7, _backward_case(256, 7, 37, 12, mode), mode)


def test_roi_align_backward_of_300_copies_of_one_roi(S, dev):
    """every RoI lands on the same pixels: the worst case for a scatter, one long ordered sum for the gather"""
    rois = np.tile(np.array([[1.0, 30.5, 21.25, 97.0, 80.5]], dtype=np.float32), (300, 1))
    _backward_run(S, dev, 256, 7, _backward_case(256, 7, 300, 77, 'copies', (rois, np.ones(300, dtype=np.int64))), 'copies')


def test_roi_align_backward_skips_rois_without_a_map(S, dev):
    """a level or an image that does not exist contributes nothing (the forward answers NaN there); K = 0 gives all-zero maps"""
    rois, levels, _ = RD.roi_cases(16, 21, 7, 2, 'mixed')
    rois, levels = rois.copy(), levels.copy()
    rois[3, 0], rois[7, 0], rois[9, 0] = 2.0, -1.0, float('nan')
    levels[5], levels[11] = 3, -1
    (tg, tr, tl), got = _backward_run(S, dev, 8, 7, _backward_case(8, 7, 16, 21, 'invalid', (rois, levels)), 'invalid')
    valid = [k for k in range(16) if k not in (3, 5, 7, 9, 11)]
    only = S.hip.roi_align_backward(tg[valid].contiguous(), RD.MAPS, RD.SCALES, tr[valid].contiguous(), tl[valid].contiguous(), 2, 2)
    assert all(torch.equal(a, b) for a, b in zip(got, only))
    empty = S.hip.roi_align_backward(torch.zeros(0, 8, 7, 7, device=dev), RD.MAPS, RD.SCALES, torch.zeros(0, 5, device=dev),
                                     torch.zeros(0, dtype=torch.int32, device=dev), 2, 2,
                                     out=[torch.full((2, h, w, 8), float('nan'), device=dev) for h, w in RD.MAPS])
    assert all(not e.any() for e in empty)
    with pytest.raises(ValueError):
        S.hip.roi_align_backward(torch.zeros(1, 12, 7, 7, device=dev), RD.MAPS, RD.SCALES, torch.zeros(1, 5, device=dev),
                                 torch.zeros(1, dtype=torch.int32, device=dev), 2, 2)


def test_roi_align_autograd_equals_the_binding(S, dev, monkeypatch):
    """`multiscale_roi_align` of maps that require grad: the forward is the kernel's, the gradient the backward binding's, and the
    switch-off route (autograd through the torch ops) agrees within the test's bound"""
    from sc2bench_amd import detection
    g, rois, levels, (want, cnt, mag) = _backward_case(8, 7, 37, 12, 'mixed')
    feats = [torch.from_numpy(f).to(dev).requires_grad_(True) for f in RD.roi_features(8, seed=8)]
    tr, tl = torch.from_numpy(rois).to(dev), torch.from_numpy(levels).to(dev)
    out = detection.multiscale_roi_align(feats, RD.SCALES, tr, tl, 7, 2)
    assert out.requires_grad
    with torch.no_grad():
        assert torch.equal(out, detection.multiscale_roi_align([f.detach() for f in feats], RD.SCALES, tr, tl, 7, 2))
    tg = torch.from_numpy(g).to(dev)
    out.backward(tg)
    direct = S.hip.roi_align_backward(tg, RD.MAPS, RD.SCALES, tr, tl.to(torch.int32), 2, 2)
    for f, d in zip(feats, direct):
        assert torch.equal(f.grad, d.permute(0, 3, 1, 2))
    kernel_grads = [f.grad.clone() for f in feats]
    monkeypatch.setattr(S.hip.host_policy, 'roi_align_bwd_hip', False)
    for f in feats:
        f.grad = None
    detection.multiscale_roi_align(feats, RD.SCALES, tr, tl, 7, 2).backward(tg)
    bound = RT.roi_backward_bound(cnt, mag)
    for l, (f, k) in enumerate(zip(feats, kernel_grads)):
        e_t = np.abs(f.grad.cpu().numpy().astype(np.float64) - want[l])
        assert np.all(e_t <= bound[l]), 'the torch-op route misses the bound on map {}'.format(l)
        print('map {}: kernel against torch ops max |diff| = {:.3e}'.format(l, (f.grad - k).abs().max().item()))


# ------------------------------------------------------------------------------------------------------------ modules
def _recorded(detection, monkeypatch, record):
    real_match, real_sampler = detection.match_boxes, detection.BalancedPositiveNegativeSampler.__call__

    def match(*args):
        out = real_match(*args)
        record.append(('match', [o.cpu() for o in out]))
        return out

    def sample(self, labels):
        record.append(('labels', [l.cpu() for l in labels]))
        pos, neg = real_sampler(self, labels)
        record.append(('sampled', [torch.where(p)[0].cpu() for p in pos] + [torch.where(n)[0].cpu() for n in neg]))
        return pos, neg
    monkeypatch.setattr(detection, 'match_boxes', match)
    monkeypatch.setattr(detection.BalancedPositiveNegativeSampler, '__call__', sample)


def _train_tail(model, feats, images, targets, seed):
    """RPN + RoI heads in training mode on fixed features -> (proposals, losses, gradients by name)"""
    for p in model.parameters():
        p.grad = None
    leaves = OrderedDict((k, v.detach().clone().requires_grad_(True)) for k, v in feats.items())
    torch.manual_seed(seed)
    proposals, rpn_losses = model.rpn(images, leaves, targets)
    _, det_losses = model.roi_heads(leaves, proposals, images.image_sizes, targets)
    losses = dict(det_losses, **rpn_losses)
    sum(losses.values()).backward()
    grads = OrderedDict((n, p.grad.detach().clone()) for n, p in model.named_parameters() if p.grad is not None)
    grads.update(('features.' + k, v.grad.detach().clone()) for k, v in leaves.items())
    return proposals, {k: v.detach() for k, v in losses.items()}, grads


def test_training_tail_on_kernels_equals_tail_on_torch_ops(S, dev, monkeypatch):
    """RegionProposalNetwork and RoIHeads in training mode on the two-level stand-in, the same seed set before each run: with the
    matcher and the RoIAlign pair on the kernels against both switches off.  Matched indices, labels, sampled index sets and
    proposals identical; each loss within 2^-12 of its value and every gradient (parameters and the feature maps) within
    2^-12 * max|grad| of the torch-op route's -- the RoIAlign bound carried through.  The observed distances are printed.
    Observed on an MI355X: the four losses identical, the gradients within 0.003 of the bound (the level-0 feature map)."""
    from sc2bench_amd import detection
    model = RT.standin_model(detection).to(dev).train()
    images = torch.stack(RT.standin_images(dev))
    targets = RT.standin_targets(dev)
    with torch.no_grad():
        feats = model.backbone(images)
    image_list = detection.ImageList(images, [RT.STANDIN_IMAGE, (RT.STANDIN_IMAGE[0] - 4, RT.STANDIN_IMAGE[1] - 8)])
    rec_k, rec_t = [], []
    _recorded(detection, monkeypatch, rec_k)
    prop_k, loss_k, grad_k = _train_tail(model, feats, image_list, targets, seed=23)
    monkeypatch.undo()
    monkeypatch.setattr(S.hip.host_policy, 'box_match_hip', False)
    monkeypatch.setattr(S.hip.host_policy, 'roi_align_bwd_hip', False)
    _recorded(detection, monkeypatch, rec_t)
    prop_t, loss_t, grad_t = _train_tail(model, feats, image_list, targets, seed=23)
    assert len(rec_k) == len(rec_t) == 6 and [r[0] for r in rec_k] == ['match', 'labels', 'sampled'] * 2
    for (kind, a), (_, b) in zip(rec_k, rec_t):
        assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)), '{} differ between the routes'.format(kind)
    assert any((m >= 0).any() for m in rec_k[0][1]) and any((m >= 0).any() for m in rec_k[3][1])      # both matchers found positives
    assert all(torch.equal(a, b) for a, b in zip(prop_k, prop_t)) and all(p.shape[0] > 0 for p in prop_k)
    for name in loss_t:
        d = (loss_k[name] - loss_t[name]).abs().item()
        print('{}: {:.6f} on torch ops, |diff| = {:.3e}'.format(name, loss_t[name].item(), d))
        assert torch.isfinite(loss_k[name]) and d <= 2.0 ** -12 * abs(loss_t[name].item())
    assert set(grad_k) == set(grad_t)
    for name in grad_t:
        top = grad_t[name].abs().max().item()
        d = (grad_k[name] - grad_t[name]).abs().max().item()
        print('grad {}: max|grad| = {:.3e}, max|diff| = {:.3e} = {:.3f} of the bound'.format(name, top, d, d / (2.0 ** -12 * top) if top else 0.0))
        assert d <= 2.0 ** -12 * top, name
    assert grad_t['features.0'].abs().max() > 0 and grad_t['features.1'].abs().max() > 0


def test_faster_rcnn_training_step(S, dev):
    """one training step end to end on the device: finite losses, a gradient on every trainable parameter, and `eval()` afterwards
    returns what it returned before the step's forward -- the training path leaves no state behind"""
    from sc2bench_amd import detection
    model = RT.standin_model(detection).to(dev)
    images, targets = RT.standin_images(dev), RT.standin_targets(dev)
    with torch.no_grad():
        before = model.eval()(images)
    torch.manual_seed(31)
    losses = model.train()(images, targets)
    assert list(losses) == ['loss_classifier', 'loss_box_reg', 'loss_objectness', 'loss_rpn_box_reg']
    assert all(torch.isfinite(v) for v in losses.values())
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, name
    with torch.no_grad():
        after = model.eval()(images)
    assert len(before) == len(after) == 2
    for a, b in zip(before, after):
        assert a['boxes'].shape[0] > 0
        for key in ('boxes', 'labels', 'scores'):
            if not torch.equal(a[key], b[key]):
                print('{}: max |diff| = {:.3e}'.format(key, (a[key].float() - b[key].float()).abs().max().item() if a[key].shape == b[key].shape else float('nan')))
            assert torch.equal(a[key], b[key]), key
