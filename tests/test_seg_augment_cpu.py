"""The PASCAL pair transforms (`custom.transform.*` of the reference's task scripts, restated in sc2bench_amd/transforms.py), their
planned form, the collate functions, `VOCSegmentation`, the config mapping and the host side of sc2_seg_augment.  No device."""
import glob
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

import seg_augment_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference/configs'
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason='reference tree not present (GPU box)')
NEW_SYMBOLS = ('sc2_seg_augment_workspace', 'sc2_seg_augment')


@pytest.fixture(scope='module')
def T():
    from sc2bench_amd import transforms
    return transforms


def pil_pair(h, w, seed=0):
    image, mask = U.source(h, w, seed)
    return Image.fromarray(image), Image.fromarray(mask)


# ------------------------------------------------------------------------------------------------ every transform alone
def test_resize_size_rule_and_square(T, monkeypatch):
    image, mask = pil_pair(37, 50)
    monkeypatch.setattr(random, 'randint', lambda a, b: 20)
    out = T.CustomRandomResize(20, 90)(image, mask)
    assert out[0].size == (27, 20) and out[1].size == (27, 20)                  # long side int(20 * 50 / 37) = 27
    assert np.array_equal(np.asarray(out[0]), np.asarray(image.resize((27, 20), Image.BILINEAR)))
    assert np.array_equal(np.asarray(out[1]), np.asarray(mask.resize((27, 20), Image.NEAREST)))
    tall = pil_pair(50, 37)
    assert T.CustomRandomResize(20)(*tall)[0].size == (20, 27)
    out = T.CustomRandomResize(20, 90, square=True)(image, mask)
    assert out[0].size == (20, 20) and out[1].size == (20, 20)
    assert T.CustomRandomResize(7).max_size == 7
    assert T._resized_hw(375, 500, 513) == (513, 684) and T._resized_hw(500, 333, 256) == (384, 256)


def test_resize_draws_between_min_and_max(T, monkeypatch):
    calls = []
    monkeypatch.setattr(random, 'randint', lambda a, b: calls.append((a, b)) or b)
    assert T.CustomRandomResize(256, 1026)(*pil_pair(7, 5))[0].size == (1026, 1436)
    assert calls == [(256, 1026)]


def test_resize_jpeg_quality_round_trip(T, monkeypatch):
    from io import BytesIO
    image, mask = pil_pair(37, 50)
    monkeypatch.setattr(random, 'randint', lambda a, b: 40)
    coded = BytesIO()
    image.save(coded, 'JPEG', quality=30)
    want = Image.open(coded).resize((54, 40), Image.BILINEAR)
    out = T.CustomRandomResize(40, 40, jpeg_quality=30)(image, mask)
    assert np.array_equal(np.asarray(out[0]), np.asarray(want))
    assert not np.array_equal(np.asarray(out[0]), np.asarray(image.resize((54, 40), Image.BILINEAR)))
    assert np.array_equal(np.asarray(out[1]), np.asarray(mask.resize((54, 40), Image.NEAREST)))       # the mask is never coded


def test_pad_if_smaller_pads_right_and_bottom(T):
    image, mask = pil_pair(7, 5)
    padded, padded_mask = T.pad_if_smaller(image, 9), T.pad_if_smaller(mask, 9, fill=255)
    assert padded.size == (9, 9) and padded_mask.size == (9, 9)
    a, m = np.asarray(padded), np.asarray(padded_mask)
    assert np.array_equal(a[:7, :5], np.asarray(image)) and (a[7:] == 0).all() and (a[:, 5:] == 0).all()
    assert np.array_equal(m[:7, :5], np.asarray(mask)) and (m[7:] == 255).all() and (m[:, 5:] == 255).all()
    assert T.pad_if_smaller(image, 5) is image                                   # min(size) >= size: untouched
    assert T.pad_if_smaller(image, 6).size == (6, 7)                             # only the side that is short grows
    t = torch.arange(6.).reshape(1, 2, 3)
    assert T.pad_if_smaller(t, 4, fill=9).shape == (1, 4, 4) and T.pad_if_smaller(t, 4, fill=9)[0, 3, 3] == 9


def test_flip_threshold(T, monkeypatch):
    image, mask = pil_pair(7, 5)
    flip = T.CustomRandomHorizontalFlip(0.5)
    monkeypatch.setattr(random, 'random', lambda: 0.5)           # random() < p is false at p itself
    out = flip(image, mask)
    assert out[0] is image and out[1] is mask
    monkeypatch.setattr(random, 'random', lambda: 0.4999)
    out = flip(image, mask)
    assert np.array_equal(np.asarray(out[0]), np.asarray(image)[:, ::-1]) and np.array_equal(np.asarray(out[1]), np.asarray(mask)[:, ::-1])


def test_crop_draws_nothing_at_exact_size(T, monkeypatch):
    def no_draw(*a, **k):
        raise AssertionError('a draw at the exact size')
    monkeypatch.setattr(torch, 'randint', no_draw)
    image, mask = pil_pair(33, 33)
    out = T.CustomRandomCrop(33)(image, mask)
    assert np.array_equal(np.asarray(out[0]), np.asarray(image))
    small = pil_pair(7, 5)
    out = T.CustomRandomCrop(9)(*small)                          # padded to exactly 9 x 9: no draw either
    assert out[0].size == (9, 9) and (np.asarray(out[1])[7:] == 255).all()
    assert T.random_crop_params(33, 33, 33, 33) == (0, 0)
    with pytest.raises(ValueError):
        T.random_crop_params(32, 40, 33, 33)


def test_crop_draws_height_then_width(T, monkeypatch):
    calls = []

    def fake(low, high, size=None, **k):
        calls.append((low, high, tuple(size)))
        return torch.tensor([high - 1])
    monkeypatch.setattr(torch, 'randint', fake)
    image, mask = pil_pair(37, 50)
    out = T.CustomRandomCrop(33)(image, mask)
    assert calls == [(0, 5, (1,)), (0, 18, (1,))]               # h - th + 1, then w - tw + 1
    assert np.array_equal(np.asarray(out[0]), np.asarray(image)[4:, 17:]) and np.array_equal(np.asarray(out[1]), np.asarray(mask)[4:, 17:])


def test_center_crop_to_tensor_normalize(T):
    image, mask = pil_pair(37, 50)
    out = T.CustomCenterCrop(21)(image, mask)
    assert np.array_equal(np.asarray(out[0]), np.asarray(image)[8:29, 14:35]) and np.array_equal(np.asarray(out[1]), np.asarray(mask)[8:29, 14:35])
    x, t = T.CustomToTensor()(image, mask)
    assert x.dtype == torch.float32 and x.shape == (3, 37, 50) and t.dtype == torch.int64 and t.shape == (37, 50)
    assert torch.equal(x, torch.from_numpy(np.array(image)).permute(2, 0, 1).float().div(255)) and int(t.max()) == 255
    kept = T.CustomToTensor(converts_sample=True, converts_target=False)(image, mask)
    assert kept[1] is mask and isinstance(kept[0], torch.Tensor)
    y, t2 = T.CustomNormalize(U.MEAN, U.STD)(x, t)
    assert t2 is t and torch.equal(y, (x - torch.tensor(U.MEAN).view(3, 1, 1)) / torch.tensor(U.STD).view(3, 1, 1))
    assert T.MISC_TRANSFORM_MODULE_DICT['CustomToTensor'] is T.CustomToTensor
    assert sorted(T.CUSTOM_TRANSFORM_DICT) == ['CustomCenterCrop', 'CustomCompose', 'CustomNormalize', 'CustomRandomCrop',
                                               'CustomRandomHorizontalFlip', 'CustomRandomResize', 'CustomToTensor']


# ------------------------------------------------------------------------------------------------ the order of the draws
def _record_draws(monkeypatch):
    calls = []
    monkeypatch.setattr(random, 'randint', lambda a, b: calls.append(('random.randint', a, b)) or 60)
    monkeypatch.setattr(random, 'random', lambda: calls.append(('random.random',)) or 0.25)

    def fake(low, high, size=None, **k):
        calls.append(('torch.randint', low, high))
        return torch.tensor([high // 2])
    monkeypatch.setattr(torch, 'randint', fake)
    return calls


def test_seeded_order_of_draws(T, monkeypatch):
    image, mask = pil_pair(37, 50)
    want = [('random.randint', 20, 90), ('random.random',), ('torch.randint', 0, 60 - 33 + 1), ('torch.randint', 0, 81 - 33 + 1)]
    calls = _record_draws(monkeypatch)
    called = U.train_chain(T)(image, mask)
    assert calls == want
    del calls[:]
    planned = U.train_chain(T).plan(image, mask)
    assert calls == want
    assert (planned.nh, planned.nw, planned.flip, planned.top, planned.left) == (60, 81, True, 14, 24)
    host = planned.host()
    assert torch.equal(host[0], called[0]) and torch.equal(host[1], called[1])


# ------------------------------------------------------------------------------------------------ plan
@pytest.mark.parametrize('form', ['train', 'eval'])
def test_plan_and_host_materialize_equal_call(T, form):
    chain = U.train_chain(T) if form == 'train' else U.eval_chain(T)
    pairs = [pil_pair(37, 50), pil_pair(50, 37), pil_pair(33, 33), pil_pair(20, 31)]
    for seed in range(6):
        U.seed_all(seed)
        called = [chain(*p) for p in pairs]
        state = random.getstate(), torch.get_rng_state()
        U.seed_all(seed)
        planned = [chain.plan(*p) for p in pairs]
        assert random.getstate() == state[0] and torch.equal(torch.get_rng_state(), state[1])      # the same draws were made
        assert all(isinstance(p, T.DeferredSegSample) and p.image.dtype == np.uint8 and p.mask.shape == p.image.shape[:2] for p in planned)
        batch = T.pascal_seg_eval_collate_fn([(p, None) for p in planned])
        assert isinstance(batch, T.DeferredSegBatch) and len(batch) == 4 and batch.buf.dtype == torch.uint8 and batch.buf.dim() == 1
        assert batch.desc.dtype == torch.int32 and tuple(batch.desc.shape) == (4, 16)
        images, targets = batch.materialize()
        want = T.pascal_seg_eval_collate_fn(called)
        assert torch.equal(images, want[0]) and torch.equal(targets, want[1]) and images.dtype == torch.float32 and targets.dtype == torch.int64
        again = batch.materialize(torch.device('cpu'))
        assert torch.equal(again[0], images)


def test_plan_refuses_other_chains(T):
    image, mask = pil_pair(37, 50)
    resize, flip, crop = T.CustomRandomResize(20, 90), T.CustomRandomHorizontalFlip(0.5), T.CustomRandomCrop(33)
    tensor, norm = T.CustomToTensor(), T.CustomNormalize(U.MEAN, U.STD)
    state = random.getstate()
    for transforms in ([T.CustomRandomResize(20, 90, jpeg_quality=50), flip, crop, tensor, norm],       # the codec stays on the host
                       [resize, crop, flip, tensor, norm],                                                # reordered
                       [flip, resize, crop, tensor, norm],
                       [resize, flip, crop, tensor],                                                      # no CustomNormalize
                       [resize, flip, crop, T.CustomToTensor(converts_target=False), norm],
                       [resize, T.CustomCenterCrop(21), tensor, norm],
                       [resize, flip, crop, norm]):
        assert T.CustomCompose(transforms).plan(image, mask) is None
    assert random.getstate() == state                                                                     # and nothing was drawn
    good = T.CustomCompose([resize, flip, crop, tensor, norm])
    assert good.plan(image, mask) is not None
    assert good.plan(image.convert('L'), mask) is None and good.plan(torch.zeros(3, 37, 50), torch.zeros(37, 50)) is None
    assert T.CustomCompose([resize, tensor, norm]).plan(image, mask) is not None
    assert T.CustomCompose([resize, crop, tensor, norm]).plan(image, mask) is not None


# ------------------------------------------------------------------------------------------------ collate functions
def test_collate_functions(T):
    chain = U.train_chain(T)
    U.seed_all(1)
    planned = [chain.plan(*pil_pair(37, 50)), chain.plan(*pil_pair(50, 37))]
    supp = ({'a': 1}, {'a': 2})
    batch = T.pascal_seg_collate_fn([(planned[0], None, supp[0]), (planned[1], None, supp[1])])
    assert isinstance(batch, T.DeferredSegBatch) and batch.extra == (supp,) and batch.size == (33, 33)
    back = batch.samples()
    assert all(np.array_equal(a.image, b.image) and np.array_equal(a.mask, b.mask) and
               (a.nh, a.nw, a.flip, a.top, a.left) == (b.nh, b.nw, b.flip, b.top, b.left) for a, b in zip(planned, back))
    # tensors go through exactly as before
    a, b = (torch.ones(3, 4, 6), torch.zeros(4, 6, dtype=torch.int64)), (torch.ones(3, 5, 3), torch.zeros(5, 3, dtype=torch.int64))
    images, targets, dicts = T.pascal_seg_collate_fn([a + (supp[0],), b + (supp[1],)])
    assert images.shape == (2, 3, 5, 6) and targets.shape == (2, 5, 6) and dicts == supp
    assert images[0, :, 4:].eq(0).all() and targets[0, 4:].eq(255).all() and targets[1, :, 3:].eq(255).all()
    images, targets = T.pascal_seg_eval_collate_fn([a, b])
    assert images.shape == (2, 3, 5, 6) and targets[1, :, 3:].eq(255).all()
    with pytest.raises(TypeError):
        T.pascal_seg_eval_collate_fn([(planned[0], None), a])
    assert T.COLLATE_FUNC_DICT['pascal_seg_collate_fn'] is T.pascal_seg_collate_fn


# ------------------------------------------------------------------------------------------------ VOCSegmentation and the configs
def test_voc_segmentation(S, T, tmp_path, monkeypatch):
    from sc2bench_amd import config as C
    assert C.resolve('torchvision.datasets.VOCSegmentation') is C.VOCSegmentation
    assert C.resolve('torchvision.datasets.ImageFolder') is C.ImageFolder and C.resolve('torchvision.datasets.CocoDetection') is C.ImageFolder
    absent = C.VOCSegmentation(str(tmp_path / 'nowhere'), download=True, transforms=U.train_chain(T))     # constructs
    with pytest.raises(FileNotFoundError):
        len(absent)
    assert isinstance(C.get_num_iterations(absent, 16), C.Placeholder)
    assert not (tmp_path / 'nowhere').exists()                                                            # download=True touched nothing
    root = tmp_path / 'voc'
    ids = U.write_voc_tree(root)
    before = sorted(str(p) for p in root.rglob('*'))
    plain = C.VOCSegmentation(str(root), year='2012', image_set='val', download=True)
    assert len(plain) == 3 and C.get_num_iterations(plain, 2) == 2
    image, target = plain[1]
    assert image.mode == 'RGB' and image.size == (37, 50) and target.size == (37, 50) and target.mode == 'P'
    assert np.array_equal(np.asarray(target), U.source(50, 37, seed=1, classes=5)[1])
    chain = U.train_chain(T)
    dataset = C.VOCSegmentation(str(root), transforms=chain)
    monkeypatch.setattr(S.hip.host_policy, 'seg_augment_hip', False)
    U.seed_all(3)
    host = [dataset[i] for i in range(3)]
    assert all(x.shape == (3, 33, 33) and t.shape == (33, 33) and t.dtype == torch.int64 for x, t in host)
    monkeypatch.setattr(S.hip.host_policy, 'seg_augment_hip', True)
    U.seed_all(3)
    planned = [dataset[i] for i in range(3)]
    assert all(isinstance(p, T.DeferredSegSample) and none is None for p, none in planned)
    images, targets = T.pascal_seg_eval_collate_fn(planned).materialize()
    assert torch.equal(images, torch.stack([x for x, _ in host])) and torch.equal(targets, torch.stack([t for _, t in host]))
    # a chain that cannot be planned is called as it is
    other = C.VOCSegmentation(str(root), transforms=T.CustomCompose([T.CustomCenterCrop(21), T.CustomToTensor()]))
    assert other[0][0].shape == (3, 21, 21)
    assert sorted(str(p) for p in root.rglob('*')) == before and len(ids) == 3


def test_data_loader_workers_hand_out_planned_samples(S, T, tmp_path):
    """two worker processes: a planned sample pickles, and no worker touches the device library"""
    from sc2bench_amd import config as C
    U.write_voc_tree(tmp_path)
    dataset = C.VOCSegmentation(str(tmp_path), transforms=U.eval_chain(T))
    loader = torch.utils.data.DataLoader(dataset, batch_size=3, num_workers=2, collate_fn=T.pascal_seg_eval_collate_fn)
    batches = list(loader)
    assert len(batches) == 1 and isinstance(batches[0], T.DeferredSegBatch)
    images, targets = batches[0].materialize()
    assert images.shape == (3, 3, 54, 54) and targets.shape == (3, 54, 54)
    want = T.pascal_seg_eval_collate_fn([U.eval_chain(T)(*dataset_pair) for dataset_pair in
                                         (C.VOCSegmentation(str(tmp_path))[i] for i in range(3))])
    assert torch.equal(images, want[0]) and torch.equal(targets, want[1])


@needs_ref
def test_reference_pascal_datasets_block_resolves(S, T):
    from sc2bench_amd import config as C
    paths = sorted(glob.glob(os.path.join(REF, 'pascal_voc2012/supervised_compression/entropic_student/*.yaml')))
    assert paths
    cfg = C.load_yaml_file(paths[0])

    def walk(obj, where):
        assert not isinstance(obj, C.Placeholder), '{} is still {!r}'.format(where, obj)
        if isinstance(obj, dict):
            for k, v in obj.items():
                walk(v, where + '/' + str(k))
        elif isinstance(obj, (list, tuple)):
            for k, v in enumerate(obj):
                walk(v, where + '/' + str(k))
        elif isinstance(obj, (C.VOCSegmentation, T.CustomCompose)):
            for k, v in vars(obj).items():
                walk(v, where + '.' + k)
    walk(cfg['datasets'], 'datasets')
    train, val = cfg['datasets']['pascal_voc2012/train'], cfg['datasets']['pascal_voc2012/val']
    assert isinstance(train, C.VOCSegmentation) and train.image_set == 'train' and isinstance(val, C.VOCSegmentation) and val.image_set == 'val'
    assert [type(t).__name__ for t in train.transforms.transforms] == ['CustomRandomResize', 'CustomRandomHorizontalFlip', 'CustomRandomCrop',
                                                                         'CustomToTensor', 'CustomNormalize']
    assert train.transforms._chain() is not None and val.transforms._chain() is not None
    assert (train.transforms.transforms[0].min_size, train.transforms.transforms[0].max_size, train.transforms.transforms[2].size) == (256, 1026, 513)


# ------------------------------------------------------------------------------------------------ ABI and the host side of the kernel
def test_symbols_switch_and_workspace(S):
    header = open(os.path.join(ROOT, 'include', 'sc2_bottleneck.h')).read()
    lib = S.hip.lib()
    for name in NEW_SYMBOLS:
        assert name in S.hip.ABI_SYMBOLS and name + '(' in header and hasattr(lib, name)
    assert lib.sc2_abi_version() == 51
    assert S.hip.HostPolicy.seg_augment_hip is True
    before = S.hip.host_policy.seg_augment_hip
    try:
        S.hip.configure(seg_augment_hip=not before)
        assert S.hip.host_policy.seg_augment_hip is (not before)
    finally:
        S.hip.configure(seg_augment_hip=before)
    assert lib.sc2_seg_augment_workspace(16, 513, 513) == 16 * 1026 * 12 * 4
    assert lib.sc2_seg_augment_workspace(0, 513, 513) == 0 and lib.sc2_seg_augment_workspace(1, 0, 5) == 0
    assert lib.sc2_seg_augment_workspace(1, S.hip.SEG_AUGMENT_MAX_SIDE + 1, 5) == 0
    with pytest.raises(S.hip.Sc2Error, match='no CPU fallback'):
        S.hip.seg_augment(torch.zeros(16, dtype=torch.uint8), np.zeros((1, 16), np.int32), (4, 4), U.MEAN, U.STD)


GOOD = dict(image_offset=0, mask_offset=6000, h=40, w=50, nh=60, nw=75, flip=1, top=10, left=20, ext_h=33, ext_w=33, pad_h=60, pad_w=75)


@pytest.mark.parametrize('field,value', [
    ('h', 0), ('w', 0), ('nh', 0), ('nw', -3), ('nh', 16385), ('w', 16385),
    ('image_offset', -1), ('image_offset', 2001), ('mask_offset', -4), ('mask_offset', 6001),
    ('flip', 2), ('flip', -1), ('ext_h', 0), ('ext_h', 34), ('ext_w', 0), ('ext_w', 34),
    ('pad_h', 59), ('pad_w', 74), ('top', -1), ('top', 28), ('left', -1), ('left', 43)])
def test_descriptor_validation_refuses(S, field, value):
    nbytes = 8000                                           # the image ends at 6000, the mask at 8000
    good = S.hip.seg_augment_desc(**GOOD)
    assert good.dtype == np.int32 and good.shape == (16,)
    S.hip.seg_augment_check(np.stack([good, good]), nbytes, 33, 33)
    bad = S.hip.seg_augment_desc(**dict(GOOD, **{field: value}))
    with pytest.raises(ValueError, match='sample 1: {} = {}'.format(field, value)):
        S.hip.seg_augment_check(np.stack([good, bad]), nbytes, 33, 33)


def test_descriptor_table_shape_and_sizes(S):
    good = S.hip.seg_augment_desc(**GOOD)
    for table, nbytes, oh, ow in ((good, 8000, 33, 33), (np.zeros((0, 16), np.int32), 8000, 33, 33), (np.stack([good])[:, :12], 8000, 33, 33),
                                  (np.stack([good]), 0, 33, 33), (np.stack([good]), 2 ** 31, 33, 33), (np.stack([good]), 8000, 0, 33),
                                  (np.stack([good]), 8000, 33, 16385)):
        with pytest.raises(ValueError):
            S.hip.seg_augment_check(table, nbytes, oh, ow)
    # the padded size defaults to what the window needs
    row = S.hip.seg_augment_desc(image_offset=0, mask_offset=30, h=2, w=5, nh=4, nw=10, flip=0, top=0, left=0, ext_h=9, ext_w=9)
    assert row[11:13].tolist() == [9, 10]
