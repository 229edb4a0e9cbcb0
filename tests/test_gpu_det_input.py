"""GPU: sc2_det_input (csrc/det_input.hip) against its numpy restatement (tests/ref_det_input.py) bit for bit -- hence within the
derived `delta` of exact-weight float64 --, its output area, its refusals, and the planned COCO batch through
`detection.GeneralizedRCNNTransform`, a training detector and `evaluate_detection`."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import det_input_cases as DC  # noqa: E402
import ref_det_input as RI  # noqa: E402
import ref_det_train as RT  # noqa: E402

pytestmark = pytest.mark.gpu

TH, TW = 16, 256      # the kernel's tile (hip.DET_INPUT_TILE_H / _W)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _launch(hip, dev, sources, sizes, flips, mean, std, Hp, Wp, lead=0, shift=16):
    """-> (out [n,3,Hp,Wp] as numpy, the arena before, the arena after, the index range of `out` in the arena)"""
    buf, offsets = DC.pack(sources, lead)
    rows = [(off, s.shape[0], s.shape[1], oh, ow, int(f)) for off, s, (oh, ow), f in zip(offsets, sources, sizes, flips)]
    numel = len(sources) * 3 * Hp * Wp
    arena = torch.full((numel + 64,), float('nan'), dtype=torch.float32, device=dev)
    out = arena[shift:shift + numel].view(len(sources), 3, Hp, Wp)
    hip.det_input(torch.from_numpy(buf).to(dev), rows, mean, std, out)
    return out.cpu().numpy(), arena.cpu().numpy(), (shift, shift + numel)


def _check_area(arena, span, out, sizes):
    lo, hi = span
    assert np.isnan(arena[:lo]).all() and np.isnan(arena[hi:]).all(), 'the launch wrote outside its output'
    assert not np.isnan(out).any(), 'an element of the output was not written'
    for i, (oh, ow) in enumerate(sizes):      # the padding is +0.0, sign bit included
        assert not _bits(out[i, :, oh:, :]).any() and not _bits(out[i, :, :, ow:]).any()


CASES = [((1, 7), (1, 7)), ((1, 7), (3, 20)), ((7, 1), (14, 2)), ((37, 53), (37, 53)), ((37, 53), (50, 71)), ((64, 64), (64, 64)),
         ((53, 37), (133, 93)), ((200, 120), (80, 48)), ((3, 667), (6, 1334)),
         # output heights and widths one below, at and one above the tile
         ((37, 53), (TH - 1, TW - 1)), ((37, 53), (TH, TW)), ((37, 53), (TH + 1, TW + 1)), ((300, 20), (2 * TH + 1, 2 * TW - 1))]


@pytest.mark.parametrize('src_hw,out_hw', CASES)
def test_kernel_equals_the_f32_restatement_bit_for_bit(S, dev, src_hw, out_hw):
    (h, w), (oh, ow) = src_hw, out_hw
    src = DC.source(h, w, seed=1)
    for flip in (False, True):
        for mean, std in ((DC.MEAN, DC.STD), (DC.ODD_MEAN, DC.ODD_STD)):
            want = RI.det_input_f32(src, oh, ow, flip, mean, std)
            exact = RI.det_input_f64(src, oh, ow, flip, mean, std)
            assert np.abs(want.astype(np.float64) - exact).max() <= RI.delta(h, w, mean, std)
            for div, shift in ((32, 16), (1, 17)):      # (the slot 16-byte aligned and not)
                Hp, Wp = DC.ceil_to(oh, div), DC.ceil_to(ow, div)
                out, arena, span = _launch(S.hip, dev, [src], [(oh, ow)], [flip], mean, std, Hp, Wp, shift=shift)
                _check_area(arena, span, out, [(oh, ow)])
                assert np.array_equal(_bits(out[0, :, :oh, :ow]), _bits(want)), \
                    '{}x{} -> {}x{} flip {} div {}: {} elements differ'.format(h, w, oh, ow, flip, div, int((_bits(out[0, :, :oh, :ow]) != _bits(want)).sum()))
                assert np.abs(out[0, :, :oh, :ow].astype(np.float64) - exact).max() <= RI.delta(h, w, mean, std)


def test_scale_one_writes_the_table_values(S, dev):
    src = DC.source(64, 64, seed=2)
    out, _, _ = _launch(S.hip, dev, [src], [(64, 64)], [False], DC.MEAN, DC.STD, 64, 64)
    table = RI.table_f32(DC.MEAN, DC.STD)
    for c in range(3):
        assert np.array_equal(_bits(out[0, c]), _bits(table[c][src[:, :, c]]))


def test_mixed_batch_in_one_launch_at_odd_offsets(S, dev):
    tr = S.detection.GeneralizedRCNNTransform(48, 80, DC.MEAN, DC.STD)
    hws = [(31, 41), (41, 31), (17, 63), (63, 17), (23, 23)]
    sources = [DC.source(h, w, seed=3 + i) for i, (h, w) in enumerate(hws)]
    sizes = [tr.resized_size(h, w) for h, w in hws]
    flips = [False, True, True, False, True]
    _, offsets = DC.pack(sources, lead=1)
    assert [o % 4 for o in offsets] == [1, 2, 3, 0, 1]      # back to back behind one leading byte: every alignment of a pixel's load
    Hp, Wp = DC.ceil_to(max(s[0] for s in sizes), 32), DC.ceil_to(max(s[1] for s in sizes), 32)
    assert len({s[0] for s in sizes}) > 1 and len({s[1] for s in sizes}) > 1      # padding on both axes, differing per sample
    out, arena, span = _launch(S.hip, dev, sources, sizes, flips, DC.MEAN, DC.STD, Hp, Wp, lead=1)
    _check_area(arena, span, out, sizes)
    assert np.array_equal(_bits(out), _bits(RI.batch_f32(sources, sizes, flips, DC.MEAN, DC.STD, Hp, Wp)))
    again, _, _ = _launch(S.hip, dev, sources, sizes, flips, DC.MEAN, DC.STD, Hp, Wp, lead=1)
    assert np.array_equal(_bits(out), _bits(again))


def test_more_samples_than_one_launch_takes(S, dev):
    n = S.hip.DET_INPUT_MAX_BATCH + 6
    hws = [(5 + i % 4, 6 + i % 3) for i in range(n)]
    sources = [DC.source(h, w, seed=100 + i) for i, (h, w) in enumerate(hws)]
    sizes = [(h + 3, w + 2) for h, w in hws]
    flips = [bool(i % 2) for i in range(n)]
    out, arena, span = _launch(S.hip, dev, sources, sizes, flips, DC.MEAN, DC.STD, 11, 10, shift=17)
    _check_area(arena, span, out, sizes)
    assert np.array_equal(_bits(out), _bits(RI.batch_f32(sources, sizes, flips, DC.MEAN, DC.STD, 11, 10)))


BAD_ROWS = [('negative offset', dict(off=-1)), ('image past the buffer', dict(off=1442)), ('zero height', dict(h=0)),
            ('width beyond the cap', dict(w=2049)), ('zero resized height', dict(oh=0)), ('resized width beyond the cap', dict(ow=2049)),
            ('negative width', dict(w=-3)), ('taller than the batch', dict(oh=41)), ('wider than the batch', dict(ow=49)),
            ('flip of 2', dict(flip=2)), ('flip of -1', dict(flip=-1))]


@pytest.mark.parametrize('what,change', BAD_ROWS, ids=[b[0] for b in BAD_ROWS])
def test_bad_rows_are_refused_before_any_launch(S, dev, what, change):
    src = DC.source(20, 24, seed=5)
    buf, _ = DC.pack([src, src], lead=1)
    good = dict(off=1, h=20, w=24, oh=30, ow=36, flip=0)
    bad = dict(good, **change)
    order = ('off', 'h', 'w', 'oh', 'ow', 'flip')
    dbuf = torch.from_numpy(buf).to(dev)
    for rows in ([bad], [good, bad]):      # alone, and behind a good row: nothing of the batch may run
        arena = torch.full((len(rows) * 3 * 40 * 48 + 32,), float('nan'), dtype=torch.float32, device=dev)
        out = arena[16:16 + len(rows) * 3 * 40 * 48].view(len(rows), 3, 40, 48)
        with pytest.raises(S.hip.Sc2Error):
            S.hip.det_input(dbuf, [[r[k] for k in order] for r in rows], DC.MEAN, DC.STD, out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(arena).all()), '{}: the arena was written'.format(what)


def test_bad_batches_are_refused(S, dev):
    src = DC.source(4, 4, seed=6)
    dbuf = torch.from_numpy(DC.pack([src])[0]).to(dev)
    out = torch.full((1, 3, 8, 8), float('nan'), device=dev)
    with pytest.raises(S.hip.Sc2Error):
        S.hip.det_input(dbuf, [[0, 4, 4, 8, 8, 0]], DC.MEAN, [0.2, 0.0, 0.2], out)      # a zero std
    with pytest.raises(S.hip.Sc2Error):
        S.hip.det_input(dbuf, [[0, 4, 4, 8, 8]], DC.MEAN, DC.STD, out)                  # a short row
    with pytest.raises(S.hip.Sc2Error):
        S.hip.det_input(dbuf.cpu(), [[0, 4, 4, 8, 8, 0]], DC.MEAN, DC.STD, out)         # a host buffer
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------------- transform level
def _planned(S, hws, flips, seed=20):
    T = S.transforms
    return T.DeferredDetBatch([T.DeferredDetSample(DC.source(h, w, seed=seed + i), f) for i, ((h, w), f) in enumerate(zip(hws, flips))])


def _targets(hws, device):
    return [{'boxes': torch.tensor([[1.0, 2.0, w - 3.0, h - 1.0], [0.0, 0.0, w / 2.0, h / 3.0]], device=device),
             'labels': torch.tensor([1, 2], device=device)} for h, w in hws]


@pytest.mark.parametrize('size_divisible', [32, 1])
def test_transform_on_a_planned_batch(S, dev, size_divisible, monkeypatch):
    T = S.transforms
    hws, flips = [(31, 41), (41, 31), (17, 63), (40, 40)], [True, False, True, False]
    tr = S.detection.GeneralizedRCNNTransform(48, 80, DC.MEAN, DC.STD, size_divisible=size_divisible).eval()
    batch = _planned(S, hws, flips)
    want, want_t = tr(batch.tensors('cpu'), _targets(hws, 'cpu'))
    exact = [RI.det_input_f64(batch[i].image, oh, ow, flips[i], DC.MEAN, DC.STD) for i, (oh, ow) in enumerate(want.image_sizes)]
    before = T.DeferredDetBatch.launches
    got, got_t = tr(batch.to(dev), _targets(hws, dev))
    assert T.DeferredDetBatch.launches == before + 1
    assert tuple(got.tensors.shape) == tuple(want.tensors.shape) and got.image_sizes == want.image_sizes
    assert got.tensors.device.type == 'cuda' and got.tensors.dtype == torch.float32
    for a, b in zip(got_t, want_t):
        assert torch.equal(a['boxes'].cpu(), b['boxes']) and torch.equal(a['labels'].cpu(), b['labels'])
    g, w = got.tensors.cpu().numpy(), want.tensors.numpy()
    for i, ((h, wd), (oh, ow)) in enumerate(zip(hws, want.image_sizes)):
        bound = RI.delta(h, wd, DC.MEAN, DC.STD)
        assert not _bits(g[i, :, oh:, :]).any() and not _bits(g[i, :, :, ow:]).any()
        err = np.abs(g[i, :, :oh, :ow].astype(np.float64) - w[i, :, :oh, :ow]).max()
        print('image {}: kernel against the host chain {:.3e}, 2 delta {:.3e}'.format(i, err, 2 * bound))
        assert err <= 2 * bound
        assert np.abs(g[i, :, :oh, :ow].astype(np.float64) - exact[i]).max() <= bound
    # an equal transform (the teacher's beside the student's) shares the result; another min_size launches once more
    twin = S.detection.GeneralizedRCNNTransform(48, 80, list(DC.MEAN), list(DC.STD), size_divisible=size_divisible).eval()
    again, _ = twin(batch, None)
    assert T.DeferredDetBatch.launches == before + 1 and again.tensors.data_ptr() == got.tensors.data_ptr()
    other, _ = S.detection.GeneralizedRCNNTransform(40, 80, DC.MEAN, DC.STD, size_divisible=size_divisible).eval()(batch, None)
    assert T.DeferredDetBatch.launches == before + 2 and other.image_sizes != got.image_sizes
    # the switch off: the present torch ops on `tensors(device)`, within delta of float64 as well, and no launch
    monkeypatch.setattr(S.hip.host_policy, 'det_input_hip', False)
    fresh = _planned(S, hws, flips).to(dev)
    off, off_t = tr(fresh, _targets(hws, dev))
    assert T.DeferredDetBatch.launches == before + 2
    assert tuple(off.tensors.shape) == tuple(want.tensors.shape) and off.image_sizes == want.image_sizes
    for a, b in zip(off_t, got_t):
        assert torch.equal(a['boxes'], b['boxes'])
    o = off.tensors.cpu().numpy()
    for i, ((h, wd), (oh, ow)) in enumerate(zip(hws, want.image_sizes)):
        assert np.abs(o[i, :, :oh, :ow].astype(np.float64) - exact[i]).max() <= RI.delta(h, wd, DC.MEAN, DC.STD)
        assert not o[i, :, oh:, :].any() and not o[i, :, :, ow:].any()


def test_tensors_on_the_device_are_the_host_chains(S, dev):
    batch = _planned(S, [(9, 13), (13, 9)], [True, False])
    for a, b in zip(batch.tensors(dev), batch.tensors('cpu')):
        assert a.device.type == 'cuda' and torch.equal(a.cpu(), b)


def test_a_slice_shares_the_copy_on_the_device(S, dev):
    hws, flips = [(31, 41), (41, 31), (17, 63)], [True, False, True]
    tr = S.detection.GeneralizedRCNNTransform(48, 80, DC.MEAN, DC.STD).eval()
    batch = _planned(S, hws, flips).to(dev)
    tr(batch)
    (device, up), = batch._on_device.items()
    tail = batch[1:]      # (what `evaluate_detection(max_samples=...)` does to the last batch)
    got, _ = tr(tail)
    assert tail._on_device is batch._on_device and len(batch._on_device) == 1 and batch._on_device[device] is up
    want, _ = tr(_planned(S, hws, flips)[1:].to(dev))      # the same samples from a buffer of their own upload
    assert got.image_sizes == want.image_sizes and torch.equal(got.tensors, want.tensors)
    batch.release()
    assert not batch._on_device and not tail._on_device
    with pytest.raises(S.hip.Sc2Error, match='not a HIP device'):
        batch.transformed(tr, 'cpu')


def test_pinned_batch_from_a_loader_gives_the_same_bits(S, dev, tmp_path):
    from sc2bench_amd import coco_data
    T = S.transforms
    img_dir, ann_file = DC.write_coco(tmp_path)
    dataset = coco_data.coco_dataset(img_dir, ann_file, annotated_only=False)
    collate = T.COLLATE_FUNC_DICT['coco_collate_fn']
    (pinned, _), = list(torch.utils.data.DataLoader(dataset, batch_size=3, collate_fn=collate, pin_memory=True))
    (plain, _), = list(torch.utils.data.DataLoader(dataset, batch_size=3, collate_fn=collate))
    assert isinstance(pinned, T.DeferredDetBatch) and pinned.buf.is_pinned() and not plain.buf.is_pinned()
    assert pinned.pin_memory() is pinned and pinned.sizes == plain.sizes == [(36, 24), (32, 32), (30, 40)]
    tr = S.detection.GeneralizedRCNNTransform(48, 80, DC.MEAN, DC.STD).eval()
    a, _ = tr(pinned.to(dev))
    b, _ = tr(plain.to(dev))
    assert a.image_sizes == b.image_sizes and torch.equal(a.tensors, b.tensors)
    assert a.tensors.data_ptr() != b.tensors.data_ptr()      # two batches: nothing is shared between them


# ----------------------------------------------------------------------------------------------------------- model level
def test_training_detector_returns_four_finite_losses_from_a_planned_batch(S, dev):
    T = S.transforms
    model = RT.standin_model(S.detection).to(dev).train()
    H, W = RT.STANDIN_IMAGE
    batch = _planned(S, [(H, W), (H, W)], [False, True], seed=30).to(dev)
    before = T.DeferredDetBatch.launches
    losses = model(batch, RT.standin_targets(dev))
    assert T.DeferredDetBatch.launches == before + 1
    assert sorted(losses) == ['loss_box_reg', 'loss_classifier', 'loss_objectness', 'loss_rpn_box_reg']
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    sum(losses.values()).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.requires_grad)


def test_evaluate_detection_over_a_coco_directory(S, dev, tmp_path):
    from sc2bench_amd import coco_data, evaluation as E
    T = S.transforms
    img_dir, ann_file = DC.write_coco(tmp_path)
    dataset = coco_data.coco_dataset(img_dir, ann_file, annotated_only=False)
    loader = torch.utils.data.DataLoader(dataset, batch_size=2, collate_fn=T.COLLATE_FUNC_DICT['coco_collate_fn'])
    assert isinstance(next(iter(loader))[0], T.DeferredDetBatch)
    model = RT.standin_model(S.detection)
    before = T.DeferredDetBatch.launches
    res = E.evaluate_detection(model, loader, dev)
    assert T.DeferredDetBatch.launches == before + 2 and res['samples'] == 3
    evaluator = res['evaluator']
    assert evaluator.img_ids == [3, 5, 7]      # the dataset's sorted ids
    assert len(res['stats']) == 12 and all(np.isfinite(res['stats']))
    for image_id, boxes, scores, labels in evaluator._preds:
        info = next(i for i in DC.COCO_IMAGES if i['id'] == image_id)
        if boxes is not None and len(boxes):      # detections are mapped back to each image's own size
            assert boxes.device.type == 'cuda'
            assert float(boxes[:, 0::2].max()) <= info['width'] and float(boxes[:, 1::2].max()) <= info['height']
