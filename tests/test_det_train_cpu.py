"""CPU: the training path of the detection tail (sc2-benchmark_amd/detection.py: matcher, sampler, box encoding, losses, the RPN and
RoI heads in training mode) and the model term of `training.WeightedSumLoss` -- all on torch ops here; tests/test_gpu_det_train.py
compares the kernels' routes against these."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_detection as RD  # noqa: E402
import ref_det_train as RT  # noqa: E402

REF = '/root/reference/configs'
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason='reference tree not present (GPU box)')


# ------------------------------------------------------------------------------------------------ box algebra, matcher, sampler
def test_box_coder_encode_then_decode_returns_the_boxes(S):
    from sc2bench_amd import detection
    g = torch.Generator().manual_seed(0)
    xy = torch.rand(40, 2, generator=g) * 100
    proposals = torch.cat([xy, xy + 4 + torch.rand(40, 2, generator=g) * 60], 1)
    xy = xy + torch.randn(40, 2, generator=g) * 3
    gt = torch.cat([xy, xy + 4 + torch.rand(40, 2, generator=g) * 60], 1)
    for weights in ((1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)):
        coder = detection.BoxCoder(weights)
        codes = coder.encode([gt[:25], gt[25:]], [proposals[:25], proposals[25:]])
        assert [tuple(c.shape) for c in codes] == [(25, 4), (15, 4)]
        back = coder.decode(torch.cat(codes), [proposals[:25], proposals[25:]])
        assert tuple(back.shape) == (40, 1, 4) and torch.allclose(back[:, 0], gt, rtol=0, atol=1e-3)
    # one pair by hand: proposal [0,0,10,20], gt [5,10,25,50]: widths 10 -> 20, heights 20 -> 40, centres (5,10) -> (15,30)
    code = detection.BoxCoder((10.0, 10.0, 5.0, 5.0)).encode_single(torch.tensor([[5.0, 10, 25, 50]]), torch.tensor([[0.0, 0, 10, 20]]))
    assert torch.allclose(code, torch.tensor([[10.0, 10.0, 5 * np.log(2.0), 5 * np.log(2.0)]]).float(), rtol=1e-6)


def test_box_iou_and_matcher_equal_the_sequential_reference(S):
    from sc2bench_amd import detection
    assert (detection.Matcher.BELOW_LOW_THRESHOLD, detection.Matcher.BETWEEN_THRESHOLDS) == (-1, -2)
    cases = [RT.match_boxes_case(300, 7, seed=1), (RD.quarter_grid_boxes(12, seed=12)[0], RD.quarter_grid_boxes(500, seed=500)[0]),
             (np.array([[5, 5, 5, 5], [0, 0, 2, 2]], dtype=np.float32), np.array([[5, 5, 5, 5], [0, 0, 2, 2]], dtype=np.float32))]
    for gt, cand in cases:
        iou = detection.box_iou(torch.from_numpy(gt), torch.from_numpy(cand))
        rows = np.stack([RT.iou_row(g, cand) for g in gt])
        assert np.array_equal(iou.numpy(), rows, equal_nan=True)
        for low, high in ((0.3, 0.7), (0.5, 0.5)):
            for allow in (False, True):
                want = RT.match_ref(gt, cand, low, high, allow)[0]
                got = detection.Matcher(high, low, allow)(iou.clone())
                assert got.dtype == torch.int64 and got.tolist() == want.tolist()
                listed = detection.match_boxes([torch.from_numpy(gt), torch.zeros(0, 4)], [torch.from_numpy(cand)] * 2, high, low, allow)
                assert listed[0].tolist() == want.tolist() and listed[1].tolist() == [-1] * len(cand)
    with pytest.raises(ValueError, match='No ground-truth'):
        detection.Matcher(0.7, 0.3)(torch.zeros(0, 5))


def test_sampler_counts_and_draw_order(S):
    from sc2bench_amd import detection
    labels = [torch.tensor([1, 0, 0, -1, 2, 0, 0, 1, 0, -1, 0, 0] * 5), torch.tensor([0, 0, 1, 0, -1, 0, 0, 0])]
    sampler = detection.BalancedPositiveNegativeSampler(16, 0.5)
    torch.manual_seed(7)
    pos, neg = sampler(labels)
    torch.manual_seed(7)      # the same draws by hand, in the order the sampler makes them: per image, positives first
    for lab, p, n in zip(labels, pos, neg):
        positive, negative = torch.where(lab >= 1)[0], torch.where(lab == 0)[0]
        num_pos = min(positive.numel(), 8)
        num_neg = min(negative.numel(), 16 - num_pos)
        want_p = positive[torch.randperm(positive.numel())[:num_pos]]
        want_n = negative[torch.randperm(negative.numel())[:num_neg]]
        assert p.dtype == torch.uint8 and torch.where(p)[0].tolist() == sorted(want_p.tolist())
        assert torch.where(n)[0].tolist() == sorted(want_n.tolist())
    assert int(pos[0].sum()) == 8 and int(neg[0].sum()) == 8          # 15 positives: capped at the fraction
    assert int(pos[1].sum()) == 1 and int(neg[1].sum()) == 6          # one positive; only six negatives exist
    assert not (pos[0] & neg[0]).any() and not (pos[0].bool() & (labels[0] < 1)).any() and not (neg[0].bool() & (labels[0] != 0)).any()


def test_smooth_l1_on_both_sides_of_beta(S):
    from sc2bench_amd import detection
    x = torch.tensor([0.0, 0.05, -0.05, 1.0 / 9, 0.5, -2.0], dtype=torch.float64)
    beta = 1.0 / 9
    each = [0.0, 0.5 * 0.05 ** 2 / beta, 0.5 * 0.05 ** 2 / beta, 1.0 / 9 - 0.5 * beta, 0.5 - 0.5 * beta, 2.0 - 0.5 * beta]
    assert detection.smooth_l1_loss(x, torch.zeros_like(x), beta=beta).item() == pytest.approx(sum(each), rel=1e-12)
    assert detection.smooth_l1_loss(x, torch.zeros_like(x), beta=beta, size_average=True).item() == pytest.approx(sum(each) / 6, rel=1e-12)
    assert detection.smooth_l1_loss(x[:0], x[:0]).item() == 0.0
    # beta = 1: torch's own
    y = torch.randn(50, 4, generator=torch.Generator().manual_seed(1))
    assert torch.allclose(detection.smooth_l1_loss(y, torch.zeros_like(y), beta=1.0), torch.nn.functional.smooth_l1_loss(y, torch.zeros_like(y), reduction='sum'))


# ------------------------------------------------------------------------------------------------ the detector in training mode
def test_training_mode_returns_losses_and_needs_targets(S):
    """a tiny FasterRCNN in training mode on CPU tensors (two 64 x 96 images, one of them without gt boxes): four finite losses,
    finite non-zero gradients on the RPN head, the box head and the backbone"""
    from sc2bench_amd import detection
    model = RT.standin_model(detection).train()
    images, targets = RT.standin_images(), RT.standin_targets()
    with pytest.raises(ValueError, match='targets should not be None'):
        model(images)
    torch.manual_seed(11)
    losses = model(images, targets)
    assert list(losses.keys()) == ['loss_classifier', 'loss_box_reg', 'loss_objectness', 'loss_rpn_box_reg']
    assert all(v.dim() == 0 and torch.isfinite(v) for v in losses.values())
    assert losses['loss_classifier'].item() == pytest.approx(np.log(RT.STANDIN_CLASSES), rel=0.05)      # near-uniform logits at initialisation
    assert losses['loss_objectness'].item() == pytest.approx(np.log(2.0), rel=0.05)
    assert losses['loss_box_reg'].item() > 0 and losses['loss_rpn_box_reg'].item() > 0
    sum(losses.values()).backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    for part in (model.rpn.head, model.roi_heads.box_head, model.roi_heads.box_predictor, model.backbone):
        assert all(p.grad.abs().max() > 0 for p in part.parameters())
    # the pieces by themselves, as the modules hand them on
    feats = model.backbone(torch.stack(images))
    image_list = detection.ImageList(torch.stack(images), [RT.STANDIN_IMAGE] * 2)
    with pytest.raises(ValueError, match='targets should not be None'):
        model.rpn(image_list, feats)
    proposals, rpn_losses = model.rpn(image_list, feats, targets)
    assert sorted(rpn_losses) == ['loss_objectness', 'loss_rpn_box_reg'] and len(proposals) == 2 and not proposals[0].requires_grad
    with pytest.raises(ValueError, match='targets should not be None'):
        model.roi_heads(feats, proposals, image_list.image_sizes)
    with pytest.raises(ValueError, match='labels key'):
        model.roi_heads(feats, proposals, image_list.image_sizes, [{'boxes': t['boxes']} for t in targets])
    result, det_losses = model.roi_heads(feats, proposals, image_list.image_sizes, targets)
    assert result == [] and sorted(det_losses) == ['loss_box_reg', 'loss_classifier']
    # eval afterwards: detections, and no loss dict
    out = model.eval()(images)
    assert len(out) == 2 and sorted(out[0]) == ['boxes', 'labels', 'scores']
    # the loss path is an opt-in per module: switched off, train() alone raises as it did before the path was built
    assert detection.enable_training(model, False) is model and not model.rpn.training_enabled and not model.roi_heads.training_enabled
    with pytest.raises(NotImplementedError, match='enable_training'):
        model.train()(images, targets)
    with pytest.raises(NotImplementedError, match='enable_training'):
        model.roi_heads(feats, proposals, image_list.image_sizes, targets)
    assert sorted(detection.enable_training(model)(images, targets)) == sorted(losses)


def test_targets_of_the_rpn_and_the_roi_heads(S):
    from sc2bench_amd import detection
    model = RT.standin_model(detection).train()
    targets = RT.standin_targets()
    anchors = model.rpn.anchor_generator(detection.ImageList(torch.zeros(2, 3, 64, 96), [RT.STANDIN_IMAGE] * 2),
                                         [torch.zeros(2, 8, 16, 24), torch.zeros(2, 8, 8, 12)])
    labels, matched = model.rpn.assign_targets_to_anchors(anchors, targets)
    assert labels[0].dtype == torch.float32 and set(labels[0].tolist()) == {-1.0, 0.0, 1.0}
    exact = torch.where((anchors[0] == targets[0]['boxes'][0]).all(1))[0]
    assert exact.numel() == 1 and labels[0][exact].item() == 1.0 and torch.equal(matched[0][exact[0]], targets[0]['boxes'][0])
    want = RT.match_ref(targets[0]['boxes'].numpy(), anchors[0].numpy(), 0.3, 0.7, True)[0]
    assert ((labels[0] == 1).numpy() == (want >= 0)).all() and ((labels[0] == -1).numpy() == (want == -2)).all()
    assert not labels[1].any() and not matched[1].any() and matched[1].shape == anchors[1].shape      # no gt boxes: all background
    # RoI heads: the gt boxes join the proposals and match themselves; background 0, ignored never (0.5 / 0.5)
    props = [torch.tensor([[8.0, 8, 40, 36], [0, 0, 10, 10], [52, 22, 88, 60]]), torch.tensor([[1.0, 1, 20, 20]])]
    torch.manual_seed(0)
    sampled, idxs, labs, reg = model.roi_heads.select_training_samples(props, targets)
    assert [p.shape[0] for p in sampled] == [5, 1] and labs[0].tolist() == [1, 0, 3, 1, 3] and labs[1].tolist() == [0]
    assert idxs[0].tolist() == [0, 0, 1, 0, 1] and reg[0][3].abs().max() == 0 and reg[0][4].abs().max() == 0      # gt against itself
    assert reg[1].shape == (1, 4)      # (encoded against a zero box, as torchvision does: -inf in dw, dh; only positive rows are ever read)


# ------------------------------------------------------------------------------------------------ criterion, stage
def _io(losses):
    return {'.': {'output': losses}}


def test_weighted_sum_loss_model_term(S):
    from sc2bench_amd import training as T
    losses = {'loss_classifier': torch.tensor(1.5), 'loss_box_reg': torch.tensor(0.25), 'loss_objectness': torch.tensor(0.5),
              'loss_rpn_box_reg': torch.tensor(0.125)}
    crit = T.build_criterion({'key': 'WeightedSumLoss', 'func2extract_model_loss': 'extract_model_loss_dict',
                              'kwargs': {'model_term': {'weight': 1.0}}})
    assert crit(_io(losses), {}, None).item() == 2.375
    assert T.WeightedSumLoss(model_term={'weight': 0.5})(_io(losses), {}, None).item() == 1.1875
    per_key = T.WeightedSumLoss(model_term={'weight': {'loss_classifier': 2.0, 'loss_rpn_box_reg': 8.0, 'loss_box_reg': 0.0, 'absent': 3.0}})
    assert per_key(_io(losses), {}, None).item() == 4.0
    # absent or zero: nothing is added and the student's output is not read
    for kwargs in ({}, {'model_term': None}, {'model_term': {'weight': 0}}, {'model_term': {}}):
        assert T.WeightedSumLoss(**kwargs)({'.': {'output': torch.zeros(3)}}, {}, None) == 0
    with pytest.raises(TypeError, match='dict of losses'):
        crit({'.': {'output': torch.zeros(3)}}, {}, None)
    with pytest.raises(KeyError, match='no_such_extractor'):
        T.WeightedSumLoss(model_term={'weight': 1.0}, func2extract_model_loss='no_such_extractor')
    # beside sub terms: the sum of both
    mse = {'feat': {'criterion': {'key': 'MSELoss', 'kwargs': {'reduction': 'sum'}}, 'weight': 2.0,
                    'criterion_wrapper': {'kwargs': {'input': {'is_from_teacher': False, 'module_path': 'a', 'io': 'output'},
                                                     'target': {'is_from_teacher': True, 'module_path': 'a', 'io': 'output'}}}}}
    s_io = dict(_io(losses), a={'output': torch.ones(4)})
    t_io = {'a': {'output': torch.zeros(4)}}
    assert T.WeightedSumLoss(sub_terms=mse)(s_io, t_io, None).item() == 8.0
    assert T.WeightedSumLoss(sub_terms=mse, model_term={'weight': 1.0})(s_io, t_io, None).item() == 10.375


def _stage2_config():
    return {'teacher': {'forward_proc': 'forward_batch_target', 'sequential': [], 'forward_hook': {'input': [], 'output': []}, 'requires_grad': False},
            'student': {'forward_proc': 'forward_batch_target', 'sequential': [], 'frozen_modules': ['backbone.conv1'],
                        'forward_hook': {'input': [], 'output': []}, 'requires_grad': True},
            'optimizer': {'key': 'SGD', 'kwargs': {'lr': 0.01, 'momentum': 0.9}},
            'criterion': {'key': 'WeightedSumLoss', 'func2extract_model_loss': 'extract_model_loss_dict', 'kwargs': {'model_term': {'weight': 1.0}}}}


def test_stage_calls_the_detector_with_batch_and_targets(S):
    """`forward_proc: 'forward_batch_target'`: student and teacher get (images, targets); the loss is the sum of the student's dict"""
    from sc2bench_amd import detection, training as T
    student, teacher = detection.enable_training(RT.standin_model(detection), False), RT.standin_model(detection, seed=6)
    stage = T.DistillationStage(teacher, student, _stage2_config(), torch.device('cpu'))
    assert student.rpn.training_enabled and student.roi_heads.training_enabled      # the stage asks for the loss dict: it opts in
    assert student.training and not teacher.training and not student.backbone.conv1.weight.requires_grad
    images, targets = RT.standin_images(), RT.standin_targets()
    torch.manual_seed(3)
    loss = stage.forward_process(images, targets)
    torch.manual_seed(3)
    want = sum(student(images, targets).values())
    assert loss.dim() == 0 and torch.isfinite(loss) and loss.item() == pytest.approx(want.item(), rel=1e-6)
    before = student.roi_heads.box_predictor.cls_score.weight.detach().clone()
    stage.post_forward_process(loss)
    assert not torch.equal(student.roi_heads.box_predictor.cls_score.weight, before)


@needs_ref
def test_reference_coco_stage2_builds(S):
    from sc2bench_amd import config as C, training as T
    path = os.path.join(REF, 'coco2017/supervised_compression/entropic_student',
                        'faster_rcnn_splittable_resnet50-fp-beta0.08_fpn_from_faster_rcnn_resnet50_fpn.yaml')
    stage = C.load_yaml_file(path)['train']['stage2']
    crit = T.build_criterion(stage['criterion'])
    assert len(crit.terms) == 0 and crit.model_loss_factor == 1.0 and crit.extract_model_loss is T.extract_model_loss_dict
    assert stage['student']['forward_proc'] == stage['teacher']['forward_proc'] == 'forward_batch_target'
    assert stage['student']['frozen_modules'] == ['backbone.body.bottleneck_layer.encoder', 'backbone.body.bottleneck_layer.entropy_bottleneck']
    losses = {'loss_classifier': torch.tensor(1.0), 'loss_box_reg': torch.tensor(2.0)}
    assert crit(_io(losses), {}, None).item() == 3.0
