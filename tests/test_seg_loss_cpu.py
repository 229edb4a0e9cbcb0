"""The segmentation training path without a device: ABI and dispatch of the loss kernels, the PASCAL criterion (`DictLossWrapper`),
`poly_lr_scheduler` stepped per iteration, `module_wise_kwargs`, `get_num_iterations`, and one CPU training step of a tiny
`BaseSegmentationModel` through `DistillationStage` with deferred resizing."""
import copy
import glob
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import ref_seg_loss as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference/configs'
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason='reference tree not present (GPU box)')
NEW_SYMBOLS = ('sc2_seg_ce_ws_bytes', 'sc2_seg_ce_forward', 'sc2_seg_ce_backward')


# ------------------------------------------------------------------------------------------------ ABI and dispatch
def test_symbols_are_declared_listed_and_exported(S):
    header = open(os.path.join(ROOT, 'include', 'sc2_bottleneck.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\b{}\s*\('.format(name), header), name
        assert name in S.hip.ABI_SYMBOLS
        assert hasattr(S.hip.lib(), name)
    lib = S.hip.lib()
    assert lib.sc2_seg_ce_ws_bytes(1, 1, 1) == 24 and lib.sc2_seg_ce_ws_bytes(8, 513, 513) == 24 * 1024
    assert lib.sc2_seg_ce_ws_bytes(0, 5, 5) == 0 and lib.sc2_seg_ce_ws_bytes(1, 5, 40000) == 0
    assert (S.hip.SEG_CE_MEAN, S.hip.SEG_CE_SUM, S.hip.SEG_CE_NONE) == (0, 1, 2)


def test_switch_exists_and_toggles(S):
    assert isinstance(S.hip.HostPolicy.seg_loss_hip, bool)
    before = S.hip.host_policy.seg_loss_hip
    try:
        S.hip.configure(seg_loss_hip=not before)
        assert S.hip.host_policy.seg_loss_hip is (not before)
    finally:
        S.hip.configure(seg_loss_hip=before)
    assert S.hip.host_policy.seg_loss_hip is before


def test_kernel_wrappers_refuse_cpu_tensors(S):
    x, t = RL.case_logits(0, 'float32'), RL.case_targets(0)
    with pytest.raises(S.hip.Sc2Error, match='no CPU fallback'):
        S.hip.seg_ce_forward(x, RL.CASES[0][3], t)
    with pytest.raises(S.hip.Sc2Error, match='no CPU fallback'):
        S.hip.seg_ce_backward(x, RL.CASES[0][3], t, torch.zeros(t.shape), torch.zeros(3, dtype=torch.float64), torch.ones(()))


@pytest.mark.parametrize('reduction', ['mean', 'sum', 'none'])
def test_cpu_tensors_take_the_torch_ops_bit_for_bit(S, reduction):
    index = 2
    size = RL.CASES[index][3]
    c = RL.CASES[index][1]
    targets = RL.case_targets(index).clone()
    targets[(targets < 0) | (targets >= c)] = RL.IGNORE
    x = RL.case_logits(index, 'float32').clone().requires_grad_(True)
    y = x.detach().clone().requires_grad_(True)
    got = S.dense.seg_cross_entropy(x, size, targets, reduction=reduction)
    want = F.cross_entropy(F.interpolate(y, size=size, mode='bilinear', align_corners=False), targets, ignore_index=255, reduction=reduction)
    assert torch.equal(got, want)
    got.sum().backward()
    want.sum().backward()
    assert torch.equal(x.grad, y.grad)
    # class weights and label smoothing reach torch too
    w = torch.rand(c, generator=torch.Generator().manual_seed(1))
    got = S.dense.seg_cross_entropy(x.detach(), size, targets, reduction=reduction, weight=w, label_smoothing=0.1)
    want = F.cross_entropy(F.interpolate(y.detach(), size=size, mode='bilinear', align_corners=False), targets, weight=w, ignore_index=255,
                           reduction=reduction, label_smoothing=0.1)
    assert torch.equal(got, want)


def test_resized_logits(S):
    x = RL.case_logits(0, 'float32')
    r = S.dense.ResizedLogits(x, torch.Size(RL.CASES[0][3]))
    assert r.logits is x and r.size == RL.CASES[0][3]
    assert torch.equal(r.resized(), F.interpolate(x, size=RL.CASES[0][3], mode='bilinear', align_corners=False))


# ------------------------------------------------------------------------------------------------ build_criterion
def _io(size=(12, 14), classes=5):
    g = torch.Generator().manual_seed(21)
    out, aux = torch.randn(2, classes, 3, 4, generator=g), torch.randn(2, classes, 6, 7, generator=g)
    targets = torch.randint(0, classes + 1, (2,) + size, generator=g)
    targets[targets == classes] = 255
    return out, aux, targets


def test_pascal_criterion_is_a_dict_loss_wrapper(S):
    from sc2bench_amd import training as T
    crit = T.build_criterion(RL.pascal_stage_config()['criterion'])
    term = crit.terms['ce']
    assert type(term) is T.DictLossWrapper and term.weights == {'out': 1.0, 'aux': 0.5}
    assert isinstance(term.low_level_loss, torch.nn.CrossEntropyLoss) and term.low_level_loss.ignore_index == 255
    out, aux, targets = _io()
    size = targets.shape[-2:]
    big = {k: F.interpolate(v, size=size, mode='bilinear', align_corners=False) for k, v in (('out', out), ('aux', aux))}
    want = 1.0 * F.cross_entropy(big['out'], targets, ignore_index=255) + 0.5 * F.cross_entropy(big['aux'], targets, ignore_index=255)
    got = crit({'.': {'output': big}}, {}, targets)
    assert torch.equal(got, want)
    deferred = {'out': S.dense.ResizedLogits(out, size), 'aux': S.dense.ResizedLogits(aux, size)}
    assert torch.equal(crit({'.': {'output': deferred}}, {}, targets), want)
    # a loss the kernels do not cover: the deferred entries are materialised
    cfg = RL.pascal_stage_config()['criterion']
    cfg['kwargs']['sub_terms']['ce']['criterion']['kwargs']['label_smoothing'] = 0.1
    smooth = T.build_criterion(cfg)
    assert not smooth.terms['ce']._fused_ce()
    want = sum(wt * F.cross_entropy(big[k], targets, ignore_index=255, label_smoothing=0.1) for k, wt in (('out', 1.0), ('aux', 0.5)))
    assert torch.equal(smooth({'.': {'output': deferred}}, {}, targets), want)


def test_wrapper_key_selects_the_class(S):
    from sc2bench_amd import training as T
    with pytest.raises(KeyError, match='NoSuchWrapper'):
        T.build_criterion(RL.pascal_stage_config(wrapper_key='NoSuchWrapper')['criterion'])
    simple = {'key': 'WeightedSumLoss', 'kwargs': {'sub_terms': {'feat': {
        'criterion': {'key': 'MSELoss', 'kwargs': {'reduction': 'sum'}},
        'criterion_wrapper': {'kwargs': {'input': {'is_from_teacher': False, 'module_path': 'a', 'io': 'output'},
                                         'target': {'is_from_teacher': True, 'module_path': 'b', 'io': 'output'}}}}}}}
    assert type(T.build_criterion(simple).terms['feat']) is T.SimpleLossWrapper      # no key: today's wrapper
    simple['kwargs']['sub_terms']['feat']['criterion_wrapper']['key'] = 'SimpleLossWrapper'
    assert type(T.build_criterion(simple).terms['feat']) is T.SimpleLossWrapper


@needs_ref
def test_reference_pascal_training_configs_build(S):
    from sc2bench_amd import config as C, training as T
    es = sorted(glob.glob(os.path.join(REF, 'pascal_voc2012/supervised_compression/entropic_student/*.yaml')))
    e2e = sorted(glob.glob(os.path.join(REF, 'pascal_voc2012/supervised_compression/end-to-end/*.yaml')))
    assert es and e2e
    for path, block in ((es[0], lambda cfg: cfg['train']['stage2']), (e2e[0], lambda cfg: cfg['train'])):
        stage = block(C.load_yaml_file(path))
        term = T.build_criterion(stage['criterion']).terms['ce']
        assert type(term) is T.DictLossWrapper and term.weights == {'out': 1.0, 'aux': 0.5} and term._fused_ce()
        assert stage['scheduler']['key'] == 'poly_lr_scheduler' and stage['scheduler']['scheduling_step'] == 1
        assert [e['module'] for e in stage['optimizer']['module_wise_kwargs']] == ['backbone', 'classifier', 'aux_classifier']
        # the dataset directory is absent here: the iteration count stays unresolved, and the scheduler says which kwarg
        n_it = stage['scheduler']['kwargs']['num_iterations']
        assert isinstance(n_it, C.Placeholder) and n_it.key == 'utils.dataset.get_num_iterations'
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
        with pytest.raises(ValueError, match='num_iterations'):
            T.poly_lr_scheduler(opt, n_it, 10)


# ------------------------------------------------------------------------------------------------ scheduler, optimizer groups
def test_poly_lr_scheduler_values(S):
    from sc2bench_amd import training as T
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.5)
    sched = T.poly_lr_scheduler(opt, num_iterations=7, num_epochs=3, power=0.9)
    assert isinstance(sched, torch.optim.lr_scheduler.LambdaLR)
    lrs = [opt.param_groups[0]['lr']]
    for _ in range(21):
        opt.step()
        sched.step()
        lrs.append(opt.param_groups[0]['lr'])
    for step in (0, 1, 20, 21):
        assert lrs[step] == pytest.approx(0.5 * (1 - step / 21.0) ** 0.9, rel=1e-12, abs=1e-15), step
    assert lrs[21] == 0.0


def _stage(S, config, lr_factor=1, model=None):
    from sc2bench_amd import training as T
    student = model if model is not None else RL.tiny_seg_model()
    teacher = RL.tiny_seg_model(seed=9)
    return T.DistillationStage(teacher, student, config, torch.device('cpu'), lr_factor=lr_factor), student


def test_scheduling_step_steps_per_iteration(S):
    images, targets = RL.tiny_batch()
    stage, _ = _stage(S, RL.pascal_stage_config(num_iterations=3, num_epochs=2, scheduling_step=1))
    base = [g['lr'] for g in stage.optimizer.param_groups]
    for it in range(1, 4):
        stage.post_forward_process(stage.forward_process(images, targets))
        factor = (1 - it / 6.0) ** 0.9
        assert [g['lr'] for g in stage.optimizer.param_groups] == pytest.approx([b * factor for b in base], rel=1e-12)
    stage.post_epoch_process()      # not per epoch as well
    assert [g['lr'] for g in stage.optimizer.param_groups] == pytest.approx([b * (1 - 3 / 6.0) ** 0.9 for b in base], rel=1e-12)
    stage.clean_modules()
    # every second optimizer step
    stage, _ = _stage(S, RL.pascal_stage_config(num_iterations=3, num_epochs=2, scheduling_step=2))
    for it in range(1, 4):
        stage.post_forward_process(stage.forward_process(images, targets))
        assert stage.optimizer.param_groups[0]['lr'] == pytest.approx(0.0025 * (1 - (it // 2) / 6.0) ** 0.9, rel=1e-12)
    stage.clean_modules()


def test_without_scheduling_step_the_scheduler_steps_per_epoch(S):
    images, targets = RL.tiny_batch()
    for absent in (None, 0):
        stage, _ = _stage(S, RL.pascal_stage_config(num_iterations=1, num_epochs=4, scheduling_step=absent))
        stage.post_forward_process(stage.forward_process(images, targets))
        stage.post_forward_process(stage.forward_process(images, targets))
        assert stage.optimizer.param_groups[0]['lr'] == 0.0025
        stage.post_epoch_process()
        assert stage.optimizer.param_groups[0]['lr'] == pytest.approx(0.0025 * (1 - 1 / 4.0) ** 0.9, rel=1e-12)
        stage.clean_modules()
    # a torch scheduler by key, as before
    cfg = RL.pascal_stage_config()
    cfg['scheduler'] = {'key': 'MultiStepLR', 'kwargs': {'milestones': [1], 'gamma': 0.1}}
    stage, _ = _stage(S, cfg)
    stage.post_forward_process(stage.forward_process(images, targets))
    assert stage.optimizer.param_groups[0]['lr'] == 0.0025
    stage.post_epoch_process()
    assert stage.optimizer.param_groups[0]['lr'] == pytest.approx(0.00025)
    stage.clean_modules()


def test_module_wise_kwargs_make_parameter_groups(S):
    stage, student = _stage(S, RL.pascal_stage_config(), lr_factor=2)
    groups = stage.optimizer.param_groups
    assert len(groups) == 3
    assert [g['initial_lr'] for g in groups] == [0.005, 0.005, 0.05]      # lr_factor scales the global and the per-group lr
    assert all(g['momentum'] == 0.9 and g['weight_decay'] == 0.0001 for g in groups)
    for group, module in zip(groups, (student.backbone, student.classifier, student.aux_classifier)):
        assert [id(p) for p in group['params']] == [id(p) for p in module.parameters()]
    assert [id(p) for p in stage.reducer.params] == [id(p) for p in student.parameters()]      # the union of the groups
    stage.clean_modules()
    stage, student = _stage(S, RL.pascal_stage_config(module_wise=False), lr_factor=2)
    assert len(stage.optimizer.param_groups) == 1 and stage.optimizer.param_groups[0]['initial_lr'] == 0.005
    assert len(stage.optimizer.param_groups[0]['params']) == len(list(student.parameters()))
    stage.clean_modules()


def test_get_num_iterations(S):
    from sc2bench_amd import config as C
    assert C.resolve('utils.dataset.get_num_iterations') is C.get_num_iterations
    data = list(range(1464))
    assert C.get_num_iterations(data, 16, 1) == 92 == math.ceil(1464 / 16)
    assert C.get_num_iterations(data, 16, 4) == 23 and C.get_num_iterations(data, 8, 3) == 61
    unresolved = C.get_num_iterations(C.Placeholder('torchvision.datasets.Nope'), 16, 1)
    assert isinstance(unresolved, C.Placeholder)


# ------------------------------------------------------------------------------------------------ one CPU training step
def test_one_training_step_with_deferred_resize(S):
    images, targets = RL.tiny_batch()
    model = RL.tiny_seg_model()
    plain = copy.deepcopy(model)
    # what forward returns today: eval mode, and training mode without the flag
    model.eval()
    with torch.no_grad():
        eval_before = model(images)
    model.train()
    with torch.no_grad():
        train_before = model(images)
    assert model.defer_resize is False
    stage, student = _stage(S, RL.pascal_stage_config(), model=model)
    assert student is model and model.defer_resize is True
    before = [p.detach().clone() for p in model.parameters()]
    loss = stage.forward_process(images, targets)
    # the undeferred model: resized logits through the same criterion
    out = plain.train()(images)
    assert all(isinstance(v, torch.Tensor) and v.shape[-2:] == images.shape[-2:] for v in out.values())
    want = F.cross_entropy(out['out'], targets, ignore_index=255) + 0.5 * F.cross_entropy(out['aux'], targets, ignore_index=255)
    assert abs(loss.item() - want.item()) <= 1e-6
    with torch.no_grad():
        deferred = model(images)
    assert all(isinstance(v, S.dense.ResizedLogits) for v in deferred.values()) and list(deferred) == ['out', 'aux']
    model.eval()
    with torch.no_grad():      # eval mode ignores the flag
        assert all(torch.equal(model(images)[k], eval_before[k]) for k in ('out', 'aux'))
    model.train()
    stage.post_forward_process(loss)
    assert all(not torch.equal(p, b) for p, b in zip(model.parameters(), before))
    stage.clean_modules()
    assert model.defer_resize is False
    # with the flag off the model and the step are what they were
    fresh = RL.tiny_seg_model().train()
    with torch.no_grad():
        now = fresh(images)
    assert all(torch.equal(now[k], train_before[k]) for k in ('out', 'aux'))


def test_defer_resize_is_left_alone_when_something_else_reads_the_output(S):
    cfg = RL.pascal_stage_config()
    cfg['student']['forward_hook'] = {'input': [], 'output': ['.']}
    stage, student = _stage(S, cfg)
    assert student.defer_resize is False
    stage.clean_modules()
    cfg = RL.pascal_stage_config()
    cfg['criterion']['kwargs']['sub_terms']['kd'] = {'criterion': {'key': 'KDLoss', 'kwargs': {}}, 'weight': 1.0}
    stage, student = _stage(S, cfg)
    assert student.defer_resize is False
    stage.clean_modules()
