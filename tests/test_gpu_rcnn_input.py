"""GPU: the two kernels of csrc/rcnn_input.hip against tests/ref_rcnn_input.py, and `RCNNTransformWithCompression`'s kernel path
against the composition of its stages.

The resize kernel is held to the rule of `ref_rcnn_input.check_resize` (the byte is the floor of the exact-weight value; where that
value is within `resize_delta` of an integer, the byte on either side of it) with at most `MARGIN_CAP` of a case's pixels decided by
the margin clause; at the input's own size it is bit-equal to `mul(255).byte()`.  The normalise-and-pad kernel is bit-equal to its
restatement.  The transform is bit-equal to: the kernel's own resized bytes -> Pillow's JPEG on the host -> `normalize_pad_ref`."""
import ctypes
import io

import numpy as np
import pytest
import torch

import ref_rcnn_input as RR

pytestmark = pytest.mark.gpu

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
ACC = [{'key': 'FileSizeAccumulator', 'kwargs': {'unit': 'KB'}}]
# (C, (H, W), (oh, ow)): the five shapes of the CPU test, one pixel, and an output of more than one 256-column tile whose width is
# no multiple of the tile or of 4 (and whose height is no multiple of the 16-row tile)
RESIZE_CASES = [(3, (7, 5), (112, 80)), (3, (37, 53), (80, 114)), (3, (53, 37), (114, 80)), (3, (20, 97), (27, 133)),
                (3, (100, 120), (80, 96)), (1, (1, 1), (5, 3)), (3, (40, 150), (37, 301))]


def _rand(C, H, W, seed=None):
    g = torch.Generator().manual_seed(H * 1000 + W if seed is None else seed)
    if H * W == 1:
        return torch.full((C, 1, 1), 0.3)
    return torch.rand(C, H, W, generator=g)


# ------------------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize('C,src,dst', RESIZE_CASES)
def test_resize_meets_the_rule(S, dev, C, src, dst):
    (H, W), (oh, ow) = src, dst
    x = _rand(C, H, W)
    got, status = S.hip.rcnn_resize_u8(x.to(dev), oh, ow)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (C, oh, ow) and got.is_contiguous()
    wrong, share = RR.check_resize(got.cpu().numpy(), RR.resize_ref(x.numpy(), oh, ow), RR.resize_delta(H, W))
    print('resize {}x{} -> {}x{}: {} wrong, margin share {:.4f}'.format(H, W, oh, ow, wrong, share))
    assert wrong == 0
    assert share <= RR.MARGIN_CAP
    assert status.item() == 0


def test_resize_reads_a_permuted_view_in_place(S, dev):
    x = _rand(3, 37, 53)
    hwc = x.permute(1, 2, 0).contiguous().to(dev)
    view = hwc.permute(2, 0, 1)
    assert not view.is_contiguous()
    a, sa = S.hip.rcnn_resize_u8(view, 80, 114)
    b, sb = S.hip.rcnn_resize_u8(x.to(dev), 80, 114)
    assert torch.equal(a, b) and sa.item() == 0 and sb.item() == 0


def test_resize_at_the_same_size_is_mul_255_byte(S, dev):
    every = (torch.arange(4096, dtype=torch.float32) % 256).div(255).reshape(1, 64, 64)
    x = torch.cat([every, torch.rand(2, 64, 64, generator=torch.Generator().manual_seed(5))])
    got, status = S.hip.rcnn_resize_u8(x.to(dev), 64, 64)
    assert torch.equal(got.cpu(), x.mul(255).byte()) and status.item() == 0


@pytest.mark.parametrize('offset', [32, 35])
def test_resize_writes_nothing_outside_its_output(S, dev, offset):
    C, (H, W), (oh, ow) = 3, (20, 97), (27, 133)
    x = _rand(C, H, W).to(dev)
    want, _ = S.hip.rcnn_resize_u8(x, oh, ow)
    n = C * oh * ow
    arena = torch.full((n + 96,), 0xA5, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = S.hip.lib().sc2_rcnn_resize_u8(ctypes.c_void_p(x.data_ptr()), H * W, W, 1, C, H, W, ctypes.c_void_p(arena.data_ptr() + offset),
                                        oh, ow, ctypes.c_void_p(status.data_ptr()), S.hip._stream())
    assert rc == 0
    arena = arena.cpu()
    assert torch.equal(arena[offset:offset + n], want.cpu().flatten())
    assert (arena[:offset] == 0xA5).all() and (arena[offset + n:] == 0xA5).all()


@pytest.mark.parametrize('value', [float('nan'), 1.5, -0.1])
@pytest.mark.parametrize('corner', ['first', 'last'])
def test_resize_reports_values_outside_the_unit_range(S, dev, value, corner):
    """one such value at a corner of the image (read by the corner lane of the first / the last tile): the status word is set, the launch
    completes; the bytes are unspecified"""
    x = _rand(3, 37, 53)
    clean, status = S.hip.rcnn_resize_u8(x.to(dev), 80, 114)
    assert status.item() == 0
    if corner == 'first':
        x[0, 0, 0] = value
    else:
        x[2, 36, 52] = value
    got, status = S.hip.rcnn_resize_u8(x.to(dev), 80, 114)
    torch.cuda.synchronize()
    assert status.item() != 0 and tuple(got.shape) == (3, 80, 114)
    # the other planes never read the value
    other = 1 if corner == 'first' else 0
    assert torch.equal(got[other], clean[other])


def test_resize_argument_errors(S, dev):
    lib, top = S.hip.lib(), S.hip.JPEG_IMAGE_MAX_SIDE
    x = torch.zeros(3, 8, 8, device=dev)
    out = torch.zeros(3 * 16 * 16, dtype=torch.uint8, device=dev)
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)      # noqa: E731

    def call(xp=None, sc=64, sh=8, sw=1, C=3, H=8, W=8, op=None, oh=16, ow=16, sp=None):
        return lib.sc2_rcnn_resize_u8(p(x) if xp is None else xp, sc, sh, sw, C, H, W, p(out) if op is None else op, oh, ow,
                                      p(st) if sp is None else sp, S.hip._stream())
    assert call() == 0
    assert call(C=2) == -2 and call(C=4) == -2
    assert call(H=0) == -2 and call(W=top + 1) == -2 and call(oh=0) == -2 and call(ow=top + 1) == -2
    null = ctypes.c_void_p(0)
    assert call(xp=null) == -1 and call(op=null) == -1 and call(sp=null) == -1
    assert call(xp=p(x, 2)) == -1 and call(sp=p(st, 2)) == -1
    assert call(sh=-8) == -1
    with pytest.raises(S.hip.Sc2Error):
        S.hip.rcnn_resize_u8(torch.zeros(2, 8, 8, device=dev), 16, 16)
    with pytest.raises(S.hip.Sc2Error):
        S.hip.rcnn_resize_u8(x, 16, top + 1)
    with pytest.raises(S.hip.Sc2Error):
        S.hip.rcnn_resize_u8(x.double(), 16, 16)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ normalise + pad
def _pixels(C, h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=(C, h, w), dtype=np.uint8)


@pytest.mark.parametrize('h,w,Hp,Wp', [(80, 114, 96, 128), (27, 133, 32, 160), (1, 1, 32, 32), (5, 7, 6, 9), (16, 256, 16, 258)])
def test_normalize_pad_is_bit_equal(S, dev, h, w, Hp, Wp):
    p = _pixels(3, h, w, seed=h + w)
    if h * w >= 256:
        p.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)      # every byte value
    slot = torch.full((3, Hp, Wp), float('nan'), device=dev)
    back = S.hip.rcnn_normalize_pad(torch.from_numpy(p).to(dev), MEAN, STD, slot)
    assert back is slot
    want = RR.normalize_pad_ref(p, MEAN, STD, Hp, Wp)
    assert (slot.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all()


def test_normalize_pad_writes_its_slot_only(S, dev):
    h, w, Hp, Wp = 27, 133, 32, 160
    p = _pixels(3, h, w, seed=3)
    batch = torch.full((3, 3, Hp, Wp), float('nan'), device=dev)
    S.hip.rcnn_normalize_pad(torch.from_numpy(p).to(dev), MEAN, STD, batch[1])
    got = batch.cpu().numpy()
    assert (got[1].view(np.uint32) == RR.normalize_pad_ref(p, MEAN, STD, Hp, Wp).view(np.uint32)).all()
    assert np.isnan(got[0]).all() and np.isnan(got[2]).all()
    one = _pixels(1, 9, 10, seed=4)       # a grey image
    slot = torch.full((1, 12, 12), float('nan'), device=dev)
    S.hip.rcnn_normalize_pad(torch.from_numpy(one).to(dev), [0.5], [0.25], slot)
    assert (slot.cpu().numpy().view(np.uint32) == RR.normalize_pad_ref(one, [0.5], [0.25], 12, 12).view(np.uint32)).all()


def test_normalize_pad_argument_errors(S, dev):
    lib = S.hip.lib()
    px = torch.zeros(3, 8, 8, dtype=torch.uint8, device=dev)
    out = torch.zeros(3 * 32 * 32 + 1, device=dev)
    m, s = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)      # noqa: E731

    def call(pp=None, C=3, h=8, w=8, mp=m, op=None, Hp=32, Wp=32):
        return lib.sc2_rcnn_normalize_pad(p(px) if pp is None else pp, C, h, w, mp, s, p(out) if op is None else op, Hp, Wp, S.hip._stream())
    assert call() == 0
    assert call(C=2) == -2 and call(h=0) == -2 and call(w=S.hip.JPEG_IMAGE_MAX_SIDE + 1) == -2 and call(Hp=4 * S.hip.JPEG_IMAGE_MAX_SIDE + 1) == -2
    assert call(Hp=7) == -1 and call(Wp=7) == -1
    null = ctypes.c_void_p(0)
    assert call(pp=null) == -1 and call(op=null) == -1 and call(mp=null) == -1 and call(op=p(out, 2)) == -1
    with pytest.raises(S.hip.Sc2Error):
        S.hip.rcnn_normalize_pad(px, MEAN, STD, torch.zeros(2, 32, 32, device=dev))
    with pytest.raises(ValueError):
        S.hip.rcnn_normalize_pad(px, MEAN, STD, torch.zeros(3, 4, 32, device=dev))      # a slot smaller than the image
    with pytest.raises(ValueError):
        S.hip.rcnn_normalize_pad(px, MEAN[:2], STD, torch.zeros(3, 32, 32, device=dev))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ the transform
def _transform(S, dev, **kw):
    codec = S.transforms.Compose([S.PILImageModule(returns_file_size=True, format='JPEG', quality=90)])
    t = S.RCNNTransformWithCompression(S.GeneralizedRCNNTransform(80, 133, MEAN, STD), dev, codec, ACC, **kw)
    t.eval()
    t.activate_analysis()
    return t


def _images(dev, sizes=((37, 53), (60, 40), (100, 120))):
    g = torch.Generator().manual_seed(1)
    return [torch.rand(3, h, w, generator=g).to(dev) for h, w in sizes]


def _composition(S, images, sizes, quality=90):
    """the kernel's own resized bytes -> Pillow's JPEG on the host -> normalize_pad_ref: (batch, file sizes)"""
    from PIL import Image
    Hp, Wp = (-(-max(s[i] for s in sizes) // 32) * 32 for i in (0, 1))
    slots, file_sizes = [], []
    for image, (oh, ow) in zip(images, sizes):
        u8, status = S.hip.rcnn_resize_u8(image, oh, ow)
        assert status.item() == 0
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(u8.cpu().numpy().transpose(1, 2, 0)), mode='RGB').save(buf, format='JPEG', quality=quality)
        file_sizes.append(len(buf.getvalue()))
        dec = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(buf.getvalue()))).transpose(2, 0, 1))
        slots.append(RR.normalize_pad_ref(dec, MEAN, STD, Hp, Wp))
    return np.stack(slots), file_sizes


def test_transform_kernel_path_equals_its_stages(S, dev, monkeypatch):
    pytest.importorskip('PIL')
    monkeypatch.setattr(S.hip.host_policy, 'rcnn_input_hip', True)
    monkeypatch.setattr(S.hip.host_policy, 'jpeg_image_hip', True)
    images = _images(dev)
    t = _transform(S, dev)
    assert t._kernel_plan(images) == (90, [(80, 114), (120, 80), (80, 96)])
    boxes = torch.tensor([[4.0, 2.0, 20.0, 30.0]], device=dev)
    out, targets = t(images, [{'boxes': boxes}, {'labels': torch.tensor([1])}, {'boxes': boxes}])
    want, file_sizes = _composition(S, images, out.image_sizes)
    assert out.image_sizes == [(80, 114), (120, 80), (80, 96)] and tuple(out.tensors.shape) == (3, 3, 128, 128)
    assert out.tensors.dtype == torch.float32 and out.tensors.device == images[0].device
    assert (out.tensors.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all()
    assert t.analyzers[0].file_size_list == [n / 1024 for n in file_sizes]
    assert torch.equal(targets[0]['boxes'].cpu(), S.detection.resize_boxes(boxes.cpu(), (37, 53), (80, 114)))
    assert 'boxes' not in targets[1] and torch.equal(targets[2]['boxes'].cpu(), S.detection.resize_boxes(boxes.cpu(), (100, 120), (80, 96)))


def test_transform_redoes_an_out_of_range_image_on_the_host(S, dev, monkeypatch):
    pytest.importorskip('PIL')
    monkeypatch.setattr(S.hip.host_policy, 'rcnn_input_hip', True)
    monkeypatch.setattr(S.hip.host_policy, 'jpeg_image_hip', True)
    images = _images(dev)
    t = _transform(S, dev)
    clean = t(images)[0].tensors.clone()
    clean_sizes = list(t.analyzers[0].file_size_list)
    t.clear_analysis()
    bad = [img.clone() for img in images]
    bad[1][1, 10, 10] = 1.5
    out = t(bad)[0]
    sizes = list(t.analyzers[0].file_size_list)
    assert torch.equal(out.tensors[0], clean[0]) and torch.equal(out.tensors[2], clean[2])
    assert len(sizes) == 3 and sizes[0] == clean_sizes[0] and sizes[2] == clean_sizes[2]
    # that image alone through the host path
    monkeypatch.setattr(S.hip.host_policy, 'rcnn_input_hip', False)
    h = _transform(S, dev)
    assert h._kernel_plan([bad[1]]) is None
    alone = h([bad[1]])[0]
    assert alone.image_sizes == [(120, 80)] and out.image_sizes[1] == (120, 80)
    assert torch.equal(out.tensors[1, :, :120, :80], alone.tensors[0, :, :120, :80])
    pad = out.tensors[1].clone()
    pad[:, :120, :80] = 0
    assert not pad.any()
    assert sizes[1] == h.analyzers[0].file_size_list[0]


class TwoMaps(torch.nn.Module):
    """a backbone without weights: the channel mean of the batch at strides 4 and 8, eight channels"""
    out_channels = 8

    def forward(self, x):
        from collections import OrderedDict
        m = x.mean(1, keepdim=True).expand(-1, 8, -1, -1)
        return OrderedDict([('0', torch.nn.functional.avg_pool2d(m, 4)), ('1', torch.nn.functional.avg_pool2d(m, 8))])


def test_model_sees_the_same_sizes_with_the_switch_on_and_off(S, dev, monkeypatch):
    pytest.importorskip('PIL')
    torch.manual_seed(0)
    detector = S.FasterRCNN(TwoMaps(), 5, min_size=80, max_size=133, box_score_thresh=0.0, rpn_post_nms_top_n_test=50,
                            rpn_anchor_generator=S.AnchorGenerator(((32,), (64,)), ((0.5, 1.0, 2.0),) * 2),
                            box_roi_pool=S.MultiScaleRoIAlign(['0', '1'], 7, 2))
    codec = S.transforms.Compose([S.PILImageModule(returns_file_size=True, format='JPEG', quality=90)])
    model = S.InputCompressionDetectionModel(detector, dev, codec_encoder_decoder=codec, analysis_config={'analyzer_configs': ACC}).to(dev).eval()
    model.activate_analysis()
    images = _images(dev)
    seen = {}
    for switch in (True, False):
        monkeypatch.setattr(S.hip.host_policy, 'rcnn_input_hip', switch)
        model.clear_analysis()
        assert (detector.transform._kernel_plan(images) is not None) is switch
        with torch.no_grad():
            batch = detector.transform(images)[0]
            model.clear_analysis()
            outputs = model(images)
        seen[switch] = (batch.image_sizes, tuple(batch.tensors.shape), [sorted(o.keys()) for o in outputs],
                        len(detector.transform.analyzers[0].file_size_list))
    assert seen[True] == seen[False]
    assert seen[True][0] == [(80, 114), (120, 80), (80, 96)] and seen[True][2] == [['boxes', 'labels', 'scores']] * 3 and seen[True][3] == 3
