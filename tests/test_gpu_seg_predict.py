"""`sc2_seg_predict` (csrc/seg.hip) on the device against tests/ref_seg.py, the float64 restatement.

Label rule (derived in tests/ref_seg.py, confirmed for these seeds on the CPU by tests/test_seg_ref_cpu.py): labels equal the
restatement's at every pixel whose float64 top-2 margin exceeds 2^-19 * max|x|; at most 1e-3 of a case's pixels fall under it.
Ties, NaN, the confusion matrix and the bytes around the buffers are exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ref_seg

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float32)


def nhwc_view(x, dev, pad_value=0.0):
    """x: CPU [N,C,h,w] -> the permuted view HipDenseHead returns: NHWC memory, channel pitch = C rounded up to 8, pad = pad_value"""
    n, c, h, w = x.shape
    pitch = (c + 7) // 8 * 8
    buf = torch.full((n, h, w, pitch), pad_value, dtype=x.dtype)
    buf[..., :c] = x.permute(0, 2, 3, 1)
    return buf.to(dev)[..., :c].permute(0, 3, 1, 2)


def sliced_view(x, dev):
    """a non-contiguous NCHW view: channels 1..C of C + 2, the first h rows of h + 1, columns 2..w+2 of w + 3, NaN around it"""
    n, c, h, w = x.shape
    big = torch.full((n, c + 2, h + 1, w + 3), float('nan'), dtype=x.dtype)
    big[:, 1:c + 1, :h, 2:w + 2] = x
    v = big.to(dev)[:, 1:c + 1, :h, 2:w + 2]
    assert not v.is_contiguous()
    return v


LAYOUTS = {'nhwc': nhwc_view, 'nchw': lambda x, dev: x.contiguous().to(dev), 'sliced': sliced_view}


@pytest.mark.parametrize('index', range(len(ref_seg.CASES)), ids=ref_seg.CASE_IDS)
def test_labels_every_layout_and_dtype(S, dev, index):
    n, c, _, size, _, _ = ref_seg.CASES[index]
    for dtype in DTYPES:
        x = ref_seg.case_logits(index, str(dtype).split('.')[1])
        for name, make in LAYOUTS.items():
            v = make(x, dev)
            assert name != 'nhwc' or (v.stride(1) == 1 and v.stride(3) == (c + 7) // 8 * 8)
            got = S.hip.seg_predict(v, size)
            assert got.shape == (n,) + size and got.dtype == torch.int64
            ref_seg.assert_labels(got, x, size, what='{} {} {}'.format(ref_seg.CASE_IDS[index], dtype, name))
            if c == 1:
                assert not got.any()


@pytest.mark.parametrize('pad', [float('nan'), 1e30], ids=['nan_pad', 'huge_pad'])
def test_pad_channels_never_take_part(S, dev, pad):
    """21 classes at pitch 24, every real logit negative: a pad channel that was read as a class would win (1e30) or poison (NaN)"""
    for index in (0, 2, 6):
        size = ref_seg.CASES[index][3]
        for dtype in DTYPES:
            x = -(ref_seg.case_logits(index, str(dtype).split('.')[1]).abs() + 0.5)
            v = nhwc_view(x, dev, pad_value=pad)
            assert v.stride(3) == 24 and v.shape[1] == 21
            got = S.hip.seg_predict(v, size)
            assert int(got.max()) < 21
            ref_seg.assert_labels(got, x, size, what='{} {} pad {}'.format(ref_seg.CASE_IDS[index], dtype, pad))


def test_exact_ties_take_the_lower_index(S, dev):
    """two identical class planes hold the maximum everywhere: the same arithmetic on the same data gives the same bits, and the
    lower index wins at every pixel, with no tolerance"""
    for index, (lo, hi) in ((0, (3, 17)), (3, (6, 9)), (6, (0, 20))):
        size = ref_seg.CASES[index][3]
        for dtype in DTYPES:
            x = ref_seg.case_logits(index, str(dtype).split('.')[1]).clone()
            x[:, lo] = x.float().abs().amax(1).to(dtype) + 1.0
            x[:, hi] = x[:, lo]
            for name, make in LAYOUTS.items():
                got = S.hip.seg_predict(make(x, dev), size)
                assert bool((got == lo).all()), (ref_seg.CASE_IDS[index], dtype, name)


def test_nan_counts_as_the_maximum(S, dev):
    index = 0
    n, c, (h, w), size, _, _ = ref_seg.CASES[index]
    for dtype in DTYPES:
        x = ref_seg.case_logits(index, str(dtype).split('.')[1]).clone()
        x[1, 7, 4, 5] = float('nan')
        y0, y1, _ = ref_seg.axis(h, size[0])
        x0, x1, _ = ref_seg.axis(w, size[1])
        touched = torch.from_numpy((((y0 == 4) | (y1 == 4))[:, None] & ((x0 == 5) | (x1 == 5))[None, :]))
        assert touched.sum() > 0
        for name, make in LAYOUTS.items():
            got = S.hip.seg_predict(make(x, dev), size).cpu()
            assert bool((got[1][touched] == 7).all()), (dtype, name)       # every pixel with the NaN among its four neighbours
            ref_seg.assert_labels(got, x, size, what='one NaN {} {}'.format(dtype, name))
        x[1, 2, 4, 5] = float('nan')      # two NaN classes at the pixel: the lower
        x[1, 12, 4, 5] = float('nan')
        for name, make in LAYOUTS.items():
            got = S.hip.seg_predict(make(x, dev), size).cpu()
            assert bool((got[1][touched] == 2).all()), (dtype, name)
            ref_seg.assert_labels(got, x, size, what='three NaN {} {}'.format(dtype, name))


@pytest.mark.parametrize('index', [0, 3, 5, 6], ids=[ref_seg.CASE_IDS[i] for i in (0, 3, 5, 6)])
def test_confusion_matrix_is_exact(S, dev, index):
    n, c, _, size, _, _ = ref_seg.CASES[index]
    targets = ref_seg.case_targets(index)
    assert {255, -1, c, c + 3, 0, c - 1} <= set(targets.flatten().tolist())
    for dtype in DTYPES:
        x = ref_seg.case_logits(index, str(dtype).split('.')[1])
        for name, make in LAYOUTS.items():
            v, t = make(x, dev), targets.to(dev)
            mat = torch.zeros(c, c, dtype=torch.int64, device=dev)
            labels = S.hip.seg_predict(v, size, t, mat)
            assert torch.equal(labels, S.hip.seg_predict(v, size))       # a target-less call: the same labels
            want = ref_seg.confusion(targets.numpy(), labels.cpu().numpy(), c)      # of the kernel's OWN labels: exact
            assert 0 < want.sum() < targets.numel()
            assert np.array_equal(mat.cpu().numpy(), want), (dtype, name)
            # a second call adds on top of the first; without labels the same counts
            assert S.hip.seg_predict(v, size, t, mat, want_labels=False) is None
            assert np.array_equal(mat.cpu().numpy(), 2 * want), (dtype, name)
            # a pre-filled matrix is kept
            pre = torch.arange(c * c, dtype=torch.int64, device=dev).reshape(c, c) * (1 << 33)
            mat2 = pre.clone()
            S.hip.seg_predict(v, size, t, mat2, want_labels=False)
            assert np.array_equal((mat2 - pre).cpu().numpy(), want), (dtype, name)
            # every target ignored: unchanged
            for ignored in (255, -1, c):
                S.hip.seg_predict(v, size, torch.full_like(t, ignored), mat2)
            assert np.array_equal((mat2 - pre).cpu().numpy(), want), (dtype, name)


def test_nothing_outside_the_declared_extents_is_written(S, dev):
    """logits inside a NaN arena, labels and matrix viewed inside sentinel buffers: the bytes around them are unchanged"""
    index = 6       # 129 x 130: partial tiles on both sides
    n, c, (h, w), (H, W), _, _ = ref_seg.CASES[index]
    sentinel = -0x0123456789ABCDEF
    targets = ref_seg.case_targets(index).to(dev)
    for dtype in DTYPES:
        x = ref_seg.case_logits(index, str(dtype).split('.')[1])
        for layout in ('nhwc', 'nchw'):
            count = n * h * w * 24 if layout == 'nhwc' else n * c * h * w
            arena = torch.full((count + 128,), float('nan'), dtype=dtype, device=dev)
            inner = arena[64:64 + count]
            if layout == 'nhwc':
                inner.view(n, h, w, 24)[..., :c] = x.permute(0, 2, 3, 1).to(dev)
                v = inner.view(n, h, w, 24)[..., :c].permute(0, 3, 1, 2)
            else:
                inner.view(n, c, h, w).copy_(x)
                v = inner.view(n, c, h, w)
            before = arena.clone()
            lab_arena = torch.full((n * H * W + 64,), sentinel, dtype=torch.int64, device=dev)
            mat_arena = torch.full((c * c + 64,), sentinel, dtype=torch.int64, device=dev)
            mat = mat_arena[32:32 + c * c].view(c, c)
            mat.zero_()
            # the library call with a caller's label buffer (hip.seg_predict allocates its own)
            labels = lab_arena[32:32 + n * H * W].view(n, H, W)
            sn, sc, sh, sw = v.stride()
            rc = S.hip.lib().sc2_seg_predict(S.hip._ptr(v), int(dtype == torch.bfloat16), n, c, h, w, sn, sc, sh, sw,
                                             24 if layout == 'nhwc' else c, H, W, S.hip._ptr(targets), S.hip._ptr(labels), S.hip._ptr(mat),
                                             S.hip._stream())
            assert rc == 0, S.hip.last_error()
            torch.cuda.synchronize(dev)
            assert torch.equal(arena.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                               before.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
            assert bool((lab_arena[:32] == sentinel).all()) and bool((lab_arena[32 + n * H * W:] == sentinel).all())
            assert bool((mat_arena[:32] == sentinel).all()) and bool((mat_arena[32 + c * c:] == sentinel).all())
            assert torch.equal(labels, S.hip.seg_predict(v, (H, W)))
            assert np.array_equal(mat.cpu().numpy(), ref_seg.confusion(targets.cpu().numpy(), labels.cpu().numpy(), c))
            ref_seg.assert_labels(labels, x, (H, W), what='arena {} {}'.format(dtype, layout))


def test_more_than_64_classes(S, dev):
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1, 65, 3, 4, generator=g)
    with pytest.raises(S.hip.Sc2Error):
        S.hip.seg_predict(x.to(dev), (10, 11))
    with pytest.raises(ValueError):
        S.hip.seg_predict(x[:, :5].to(dev), (10, 11), want_labels=False)      # nothing to compute
    targets = torch.randint(0, 65, (1, 10, 11), generator=g)
    ev = S.dense.SegEvaluator(65)
    ev.update_logits(targets.to(dev), x.to(dev))       # falls back to torch ops
    want = S.dense.SegEvaluator(65)
    want.update(targets.to(dev).flatten(), F.interpolate(x.to(dev), size=(10, 11), mode='bilinear', align_corners=False).argmax(1).flatten())
    assert torch.equal(ev.mat, want.mat) and int(ev.mat.sum()) == targets.numel()
    # and 64 classes through the evaluator: the kernel
    ev64 = S.dense.SegEvaluator(64)
    x64 = ref_seg.case_logits(3, 'float32')
    t64 = ref_seg.case_targets(3)
    ev64.update_logits(t64.to(dev), x64.to(dev))
    labels = S.hip.seg_predict(x64.to(dev), ref_seg.CASES[3][3])
    assert np.array_equal(ev64.mat.cpu().numpy(), ref_seg.confusion(t64.numpy(), labels.cpu().numpy(), 64))


def test_model_predict(S, dev):
    """DeepLabv3 in bf16 eval (the `seg513` workload's model): predict = the restatement on the classifier's low-resolution logits,
    = the torch-op path exactly with the switch off; forward does not change with the switch"""
    import bench
    torch.manual_seed(0)
    model = bench.build_workload('seg513', dev, 1)[0]
    x = torch.rand(1, 3, 257, 257, generator=torch.Generator().manual_seed(14)).to(dev)
    g = torch.Generator().manual_seed(15)
    targets = torch.randint(0, 22, (1, 257, 257), generator=g)
    targets[targets == 21] = 255
    with torch.no_grad():
        logits = model._logits(model.classifier, model.backbone(x)['out'])
        assert logits.dtype == torch.bfloat16 and logits.shape[:2] == (1, 21) and logits.stride(1) == 1 and logits.stride(3) == 24
        mat = torch.zeros(21, 21, dtype=torch.int64, device=dev)
        labels = model.predict(x, targets.to(dev), mat)
        out_on = model(x)['out']
        assert labels.shape == (1, 257, 257) and labels.dtype == torch.int64
        ref_seg.assert_labels(labels, logits.cpu(), (257, 257), what='deeplabv3 predict')
        assert np.array_equal(mat.cpu().numpy(), ref_seg.confusion(targets.numpy(), labels.cpu().numpy(), 21))
        S.hip.configure(seg_predict_hip=False)
        try:
            mat_off = torch.zeros(21, 21, dtype=torch.int64, device=dev)
            labels_off = model.predict(x, targets.to(dev), mat_off)
            out_off = model(x)['out']
        finally:
            S.hip.configure(seg_predict_hip=True)
        want_off = F.interpolate(logits.float(), size=(257, 257), mode='bilinear', align_corners=False).argmax(1)
        assert torch.equal(labels_off, want_off)
        assert np.array_equal(mat_off.cpu().numpy(), ref_seg.confusion(targets.numpy(), labels_off.cpu().numpy(), 21))
        assert out_on.dtype == out_off.dtype and torch.equal(out_on.view(torch.int16), out_off.view(torch.int16))
        assert out_on.shape == (1, 21, 257, 257)


def test_evaluate_segmentation_takes_a_model_from_the_host(S, dev):
    """an updated model that still lives on the host (what `test_only` builds from a config): evaluate_segmentation moves it to the
    device BEFORE it enters inference mode (buffers copied under inference mode track no version, and the coder's table cache keys
    on versions), runs the coder path per batch and counts what `predict` labels"""
    import bench
    from sc2bench_amd import evaluation
    torch.manual_seed(0)
    model = bench.build_workload('seg513', dev, 1)[0].cpu()
    g = torch.Generator().manual_seed(16)
    data = [(torch.rand(3, h, w, generator=g), torch.randint(0, 21, (h, w), generator=g)) for h, w in ((257, 257), (241, 249))]
    loader = evaluation.build_data_loader({'val': data}, {'dataset_id': 'val', 'kwargs': {'batch_size': 2},
                                                         'collate_fn': 'pascal_seg_eval_collate_fn'})
    res = evaluation.evaluate_segmentation(model, loader, dev, 21)
    assert next(model.parameters()).is_cuda and res['samples'] == 2
    images, targets = S.transforms.pascal_seg_eval_collate_fn(data)
    assert int((targets == 255).sum()) == 257 * 257 - 241 * 249
    with torch.no_grad():
        labels = model.predict(images.to(dev))
    want = ref_seg.confusion(targets.numpy(), labels.cpu().numpy(), 21)
    assert np.array_equal(res['evaluator'].mat.cpu().numpy(), want) and want.sum() == 257 * 257 + 241 * 249

